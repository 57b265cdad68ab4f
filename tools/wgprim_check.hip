// tools/wgprim_check.hip -- the workgroup primitives of csrc/wgprim.h one by one against a host loop (tests/test_wgprim_gpu.py runs it):
//   * wg_scan_array   n = 0 .. 70001 (empty, a partial wave, one element per thread, a ragged last run, many elements per thread);
//                     int32 -> int32 from 0, int32 -> int64 behind a non-zero base with a total past 2^31, and int32 in place
//                     (off = cnt) at n = 2049: three elements per thread and a ragged last run
//   * wg_scan_incl    256 and 1024 threads; int32, uint32, int64; zeros, ones, alternating, a single one in the last lane, random
//   * wg_rank         256 and 1024 threads, the same flag patterns
// wg_scan_incl and wg_rank run twice in a row on the same LDS words (the trailing barrier).  Exact integer equality throughout.
// Prints one line per check and "ALL OK" at the end; exit code 1 on the first mismatch or failed HIP call.
#include "../reconstructor_amd/csrc/wgprim.h"
#include <cstdio>
#include <vector>

#define CK(call)                                                                                    \
    do {                                                                                            \
        const hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) { printf("%s: %s  FAILED\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)

static unsigned long long rnd(unsigned long long &x)
{
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    return x;
}

template <typename TO>
__global__ __launch_bounds__(1024) void k_array(const int32_t *cnt, long n, TO *off, TO base, TO *ret)
{
    ret[threadIdx.x] = wg_scan_array(cnt, n, off, base);
}

template <typename T, int NT>
__global__ __launch_bounds__(NT) void k_incl(const T *v, T *out, T *tot)
{
    __shared__ T sh[NT / 64];
    const int t = threadIdx.x;
    for (int r = 0; r < 2; ++r) out[r * NT + t] = wg_scan_incl<T, NT>(v[r * NT + t], sh, tot[r * NT + t]);
}

template <int NT>
__global__ __launch_bounds__(NT) void k_rank(const uint8_t *flag, int *out, int *tot)
{
    __shared__ int sh[NT / 64];
    const int t = threadIdx.x;
    for (int r = 0; r < 2; ++r) out[r * NT + t] = wg_rank<NT>(flag[r * NT + t] != 0, sh, tot[r * NT + t]);
}

static const char *const kPattern[5] = {"zeros", "ones", "alternating", "one in the last lane", "random"};

// value of thread t under pattern p (`big`: the largest random value)
static unsigned long long pattern(int p, int t, int nt, unsigned long long big, unsigned long long &seed)
{
    switch (p) {
    case 0: return 0;
    case 1: return 1;
    case 2: return (unsigned long long)(t & 1);
    case 3: return t == nt - 1 ? 1 : 0;
    default: return rnd(seed) % (big + 1);
    }
}

template <typename TO>
static int check_array(const char *name, TO base, int32_t max_cnt, int32_t *d_cnt, void *d_off, void *d_ret)
{
    const TO guard = (TO)-77;
    unsigned long long seed = 88172645463325252ull;
    for (long n : {0L, 1L, 63L, 64L, 65L, 1023L, 1024L, 1025L, 2047L, 2049L, 70001L}) {
        std::vector<int32_t> cnt((size_t)n + 1);
        for (auto &c : cnt) c = (int32_t)(rnd(seed) % ((unsigned long long)max_cnt + 1));
        std::vector<TO> off((size_t)n + 1, guard), ret(1024);
        CK(hipMemcpy(d_cnt, cnt.data(), cnt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        CK(hipMemcpy(d_off, off.data(), off.size() * sizeof(TO), hipMemcpyHostToDevice));      // off[n] is not the function's to write
        k_array<TO><<<1, 1024>>>(d_cnt, n, (TO *)d_off, base, (TO *)d_ret);
        CK(hipGetLastError());
        CK(hipMemcpy(off.data(), d_off, off.size() * sizeof(TO), hipMemcpyDeviceToHost));
        CK(hipMemcpy(ret.data(), d_ret, ret.size() * sizeof(TO), hipMemcpyDeviceToHost));
        TO run = base;
        long bad = 0;
        for (long i = 0; i < n; ++i) { bad += off[i] != run; run += cnt[i]; }
        bad += off[n] != guard;
        for (int t = 0; t < 1024; ++t) bad += ret[t] != run;
        printf("wg_scan_array %s, n = %5ld, total %lld: %ld wrong  %s\n", name, n, (long long)run, bad, bad ? "FAILED" : "ok");
        if (bad) return 1;
    }
    return 0;
}

template <typename T, int NT>
static int check_incl(const char *name, unsigned long long big, void *d_in, void *d_out, void *d_tot)
{
    unsigned long long seed = 1442695040888963407ull;
    for (int p = 0; p < 5; ++p) {
        std::vector<T> v(2 * NT), out(2 * NT), tot(2 * NT);
        for (int t = 0; t < NT; ++t) v[t] = (T)pattern(p, t, NT, big, seed);
        for (int t = 0; t < NT; ++t) v[NT + t] = (T)pattern(4, t, NT, big, seed);               // the second call: other values on the same words
        CK(hipMemcpy(d_in, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xA5, 2 * NT * sizeof(T)));
        CK(hipMemset(d_tot, 0xA5, 2 * NT * sizeof(T)));
        k_incl<T, NT><<<1, NT>>>((const T *)d_in, (T *)d_out, (T *)d_tot);
        CK(hipGetLastError());
        CK(hipMemcpy(out.data(), d_out, out.size() * sizeof(T), hipMemcpyDeviceToHost));
        CK(hipMemcpy(tot.data(), d_tot, tot.size() * sizeof(T), hipMemcpyDeviceToHost));
        int bad = 0;
        for (int r = 0; r < 2; ++r) {
            T run = 0, sum = 0;
            for (int t = 0; t < NT; ++t) sum += v[r * NT + t];
            for (int t = 0; t < NT; ++t) { run += v[r * NT + t]; bad += out[r * NT + t] != run; bad += tot[r * NT + t] != sum; }
        }
        printf("wg_scan_incl %s x %4d, %s then random: %d wrong  %s\n", name, NT, kPattern[p], bad, bad ? "FAILED" : "ok");
        if (bad) return 1;
    }
    return 0;
}

template <int NT>
static int check_rank(uint8_t *d_flag, int *d_out, int *d_tot)
{
    unsigned long long seed = 6364136223846793005ull;
    for (int p = 0; p < 5; ++p) {
        std::vector<uint8_t> f(2 * NT);
        std::vector<int> out(2 * NT), tot(2 * NT);
        for (int t = 0; t < NT; ++t) f[t] = (uint8_t)pattern(p, t, NT, 1, seed);
        for (int t = 0; t < NT; ++t) f[NT + t] = (uint8_t)pattern(4, t, NT, 1, seed);
        CK(hipMemcpy(d_flag, f.data(), f.size(), hipMemcpyHostToDevice));
        CK(hipMemset(d_out, 0xA5, 2 * NT * sizeof(int)));
        CK(hipMemset(d_tot, 0xA5, 2 * NT * sizeof(int)));
        k_rank<NT><<<1, NT>>>(d_flag, d_out, d_tot);
        CK(hipGetLastError());
        CK(hipMemcpy(out.data(), d_out, out.size() * sizeof(int), hipMemcpyDeviceToHost));
        CK(hipMemcpy(tot.data(), d_tot, tot.size() * sizeof(int), hipMemcpyDeviceToHost));
        int bad = 0;
        for (int r = 0; r < 2; ++r) {
            int below = 0, sum = 0;
            for (int t = 0; t < NT; ++t) sum += f[r * NT + t];
            for (int t = 0; t < NT; ++t) { bad += out[r * NT + t] != below; bad += tot[r * NT + t] != sum; below += f[r * NT + t]; }
        }
        printf("wg_rank x %4d, %s then random: %d wrong  %s\n", NT, kPattern[p], bad, bad ? "FAILED" : "ok");
        if (bad) return 1;
    }
    return 0;
}

// off = cnt: every thread reads its run before it writes it
static int check_in_place(int32_t *d_cnt, int32_t *d_ret)
{
    const long n = 2049;
    unsigned long long seed = 2862933555777941757ull;
    std::vector<int32_t> cnt((size_t)n + 1), got((size_t)n + 1), ret(1024);
    for (auto &c : cnt) c = (int32_t)(rnd(seed) % 16);
    CK(hipMemcpy(d_cnt, cnt.data(), cnt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    k_array<int32_t><<<1, 1024>>>(d_cnt, n, d_cnt, 7, d_ret);
    CK(hipGetLastError());
    CK(hipMemcpy(got.data(), d_cnt, got.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    CK(hipMemcpy(ret.data(), d_ret, ret.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    int32_t run = 7;
    long bad = 0;
    for (long i = 0; i < n; ++i) { bad += got[i] != run; run += cnt[i]; }
    bad += got[n] != cnt[n];                                    // the word behind the array is left alone
    for (int t = 0; t < 1024; ++t) bad += ret[t] != run;
    printf("wg_scan_array int32 in place from 7, n = %5ld, total %d: %ld wrong  %s\n", n, run, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main()
{
    const size_t nmax = 70001 + 1;
    int32_t *d_cnt;
    void *d_a, *d_b, *d_c;                          // 8-byte words: enough for every check below
    CK(hipMalloc(&d_cnt, nmax * sizeof(int32_t)));
    CK(hipMalloc(&d_a, nmax * 8));
    CK(hipMalloc(&d_b, nmax * 8));
    CK(hipMalloc(&d_c, nmax * 8));
    if (check_array<int32_t>("int32 -> int32 from 0", 0, 15, d_cnt, d_a, d_b)) return 1;
    if (check_array<int64_t>("int32 -> int64 from 5000000000", 5000000000ll, 1 << 21, d_cnt, d_a, d_b)) return 1;
    if (check_in_place(d_cnt, (int32_t *)d_b)) return 1;
    if (check_incl<int32_t, 256>("int32", 1u << 20, d_a, d_b, d_c)) return 1;
    if (check_incl<int32_t, 1024>("int32", 1u << 20, d_a, d_b, d_c)) return 1;
    if (check_incl<uint32_t, 256>("uint32", 0xFFFFFFFFull, d_a, d_b, d_c)) return 1;            // wraps: unsigned sums are exact modulo 2^32
    if (check_incl<uint32_t, 1024>("uint32", 0xFFFFFFFFull, d_a, d_b, d_c)) return 1;
    if (check_incl<int64_t, 256>("int64", 1ull << 40, d_a, d_b, d_c)) return 1;
    if (check_incl<int64_t, 1024>("int64", 1ull << 40, d_a, d_b, d_c)) return 1;
    if (check_rank<256>((uint8_t *)d_a, (int *)d_b, (int *)d_c)) return 1;
    if (check_rank<1024>((uint8_t *)d_a, (int *)d_b, (int *)d_c)) return 1;
    CK(hipDeviceSynchronize());
    CK(hipFree(d_cnt)); CK(hipFree(d_a)); CK(hipFree(d_b)); CK(hipFree(d_c));
    printf("ALL OK\n");
    return 0;
}
