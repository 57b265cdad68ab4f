// chol.hip -- K7: dense blocked FP64 Cholesky on MI355X (gfx950) with its own multi-stream scheduler, and the triangular
// solves behind it.  Host interface: chol.h (its user is ba.hip, the reduced camera system); the schedule as data: chol_plan.h.
//
// Kernels:
//   K7 k_chol_diag -> k_gemm_q<0> -> k_gemm_q<1> (latency chain) beside k_gemm_nt_pipe (panels and columns on a second
//      stream, bulk updates on a third): blocked right-looking Cholesky, v_mfma_f64_16x16x4_f64   [f64 MFMA]
//      k_trsv_bwd_chain (k_trsv_bwd per step as its fallback; k_trsv_fwd only when the rhs does not ride through the factorisation)
// The kernels take raw pointers only; nothing here knows what the system is made of.
#include "rcn_internal.h"

#include <chrono>
#include <cstdlib>
#include <utility>

#define NB chol::BLOCK        // Cholesky block size

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// one thread: relaxed poll (an sc1 load) with a 2-second limit (100 MHz wall clock, independent of the shader clock)
#ifdef RCN_DIAG
// Diagnostic build only: a device-side timeline of the factorisation's kernels (tools/chol_device_timeline.py).  rocprofv3's kernel
// trace stretches dependent launches and cross-stream hand-offs by tens of microseconds, which is the very thing to be measured.
// Slot 3 * id: first workgroup entered; + 1: its gate passed; + 2: last workgroup left.  id = 8 * block step + kind.
__device__ unsigned long long *g_tl = nullptr;
#define TL_MARK(id, w) do { if (g_tl && threadIdx.x == 0 && (blockIdx.x == 0 || (w) == 2)) atomicMax(&g_tl[3 * (id) + (w)], (unsigned long long)wall_clock64()); } while (0)
extern "C" int rcn_diag_timeline_set(unsigned long long *dev_buf)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(g_tl), &dev_buf, sizeof(dev_buf)) == hipSuccess ? 0 : -1;
}
#else
#define TL_MARK(id, w)
#endif
// The flag word is STICKY: the first event of a factorisation owns it (0 -> code by compare-and-swap), so a gate timeout (3) is
// never overwritten by the non-finite pivot (1) that the kernels behind it may then meet on half-updated tiles -- the host must
// see the 3 to switch schedules -- and a wait that finds the flag already raised returns at once: the result is discarded
// anyway, and every later hand-off of the same factorisation would otherwise burn its own 2 s.
__device__ __forceinline__ void flag_raise(int *flag, int code)
{
    (void)atomicCAS(flag, 0, code);
}
#ifdef RCN_DIAG
__device__ int g_poll[2] = {0, 1};      // {the time-out by the clock (0) or by a count of polls (1), s_sleep(8) per poll}: tools/ only
extern "C" int rcn_diag_set_poll(int mode, int sleeps)
{
    const int h[2] = {mode, sleeps};
    return hipMemcpyToSymbol(HIP_SYMBOL(g_poll), h, sizeof(h)) == hipSuccess ? 0 : -1;
}
#endif
__device__ __forceinline__ void ring_wait(const int *counter, int need, int *flag, int code = 3)
{
#ifdef RCN_DIAG
    const int mode = g_poll[0], sleeps = g_poll[1];
#else
    const int mode = 0, sleeps = 1;
#endif
    const unsigned long long t0 = mode == 0 ? wall_clock64() : 0ull;
    unsigned spins = 0;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < need) {
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
        for (int q = 0; q < sleeps; ++q) __builtin_amdgcn_s_sleep(8);
        if (mode == 0 ? wall_clock64() - t0 > 200000000ull : ++spins > 2000000u) { flag_raise(flag, code); break; }
    }
}

// Cross-stream hand-offs of the factorisation: every stream owns counters that say how far it has come, and a kernel
// that needs another stream's result waits for the counter itself.
//   publish  a kernel's first thread stores the counter of the work that PRECEDES it on its stream: stream order has
//            completed that work and the kernel boundary has released its writes, so the store needs no fence and costs
//            the publishing stream nothing (a trailing signal kernel would cost ~5 us of the chain per step);
//   wait     thread 0 of every workgroup polls (relaxed), then ONE agent-scope acquire, then the workgroup barrier:
//            the consumer recipe of MI355X_MICROARCH.md (inter-workgroup visibility), after which plain loads are safe.
struct Gate { const int *c[6]; int n[6]; int nw; int *pub; int pubval; int *flag; };
__host__ __device__ inline Gate gate_none(int *flag)
{
    Gate g = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {0, 0, 0, 0, 0, 0}, 0, nullptr, 0, flag};
    return g;
}
__device__ __forceinline__ void gate_enter(const Gate &g)
{
    if (threadIdx.x == 0) {
        if (g.pub && blockIdx.x == 0) __hip_atomic_store(g.pub, g.pubval, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g.nw > 0) ring_wait(g.c[0], g.n[0], g.flag);
        if (g.nw > 1) ring_wait(g.c[1], g.n[1], g.flag);
        if (g.nw > 2) ring_wait(g.c[2], g.n[2], g.flag);
        if (g.nw > 3) ring_wait(g.c[3], g.n[3], g.flag);
        if (g.nw > 4) ring_wait(g.c[4], g.n[4], g.flag);
        if (g.nw > 5) ring_wait(g.c[5], g.n[5], g.flag);
        if (g.nw > 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    if (g.nw > 0) __syncthreads();
}

__global__ __launch_bounds__(64) void k_ring_gate(Gate g)
{
    gate_enter(g);
}
#ifdef RCN_DIAG
// RCN_CHOL_BREAK=2 (diagnostic build): what a broken hand-off does to the numbers -- the diagonal block behind it holds garbage
__global__ void k_diag_poison(double *S, int ld, int kb)
{
    S[((size_t)kb * NB) * ld + (size_t)kb * NB] = __longlong_as_double(0x7ff8000000000000ll);
}
#endif

// ---------------------------------------------------------------------------------------
// K7: dense Cholesky of the padded reduced system (npad multiple of 128), lower triangle.
// Diagonal block (one workgroup of eight waves, block resident in LDS, 16 workgroup barriers in total):
//   1. blocked factorisation with 16-wide leaves.  A leaf is factored AND inverted by wave 0 alone, on the matrix pipe
//      (leaf_factor below); rows below become A Dinv^T and the trailing square is updated as 16x16
//      v_mfma_f64_16x16x4_f64 tiles.  Lookahead: wave 0 updates the next leaf's diagonal tile first and factors it
//      while waves 1..7 finish the trailing square, so the serial leaf work hides behind the MFMA work;
//   2. the inverse of the factor grows a block row per leaf in the same phase, by waves 1..7, also behind the leaf:
//          Linv[k][j] = -Dinv_k * sum_{m = j .. k-1} L[k][m] Linv[m][j]
//      (round 2 inverted by doubling, 16 -> 32 -> 64 -> 128, AFTER the factorisation: 11 us of the kernel's 58).
//      Leaf inverses sit in place on the diagonal (the factor's own leaf blocks wait transposed above it, diagonal in rd);
//      the other inverse blocks sit in the mirror position above the diagonal, the factor stays below it.
// Writes L^-1 into Linv[kb] (used by the panel GEMM and the triangular solves) as it appears and, on request, L into S.
#define DL 129   // LDS row stride of the diagonal block (doubles): row walks are conflict-free
#define LB 16    // leaf size
#ifdef RCN_STAMP   // diagnostic build only (tools/chol_diag_bench.hip): phase time stamps
__device__ unsigned long long g_stamps[64];
#define STAMP(i) do { __syncthreads(); if (threadIdx.x == 0) g_stamps[i] = clock64(); } while (0)
#else
#define STAMP(i)
#endif
// ring_done / ring_need: in the chain-bound steps of the factorisation (the host decides) this kernel also does the gate's
// job on its way out -- by then the bulk update the first trailing column of this step waits for has long finished, so
// the check is free and the chain loses a 5-us kernel; ring_need < 0: nothing to wait for here.
#define CDW 8          // waves of the diagonal kernel: wave 0 owns the leaves, the others the matrix work between them.  Eight since the
                       // leaf moved to the matrix pipe (136 registers; the vector-ALU leaf of round 2 wanted ~340 and spilled at
                       // eight waves); the doubling steps (2c) deal their tiles to exactly eight waves
// nact: the block's ACTIVE rows -- below them it is the identity padding of the system (the last block of every factorisation; the only
// block of the reference's own problem sizes: 3 cameras are 13 rows of 128).  Only the leaves that hold active rows are factored; the
// rest of the block is its own factor and inverse, and is written as such.
// (the body: k_chol_diag = one block per launch on the chain's stream; k_chol_diag_server = every block of a factorisation in ONE
//  resident workgroup -- round 5, below.  false: a pivot broke down, flag 1 is raised)
__device__ __forceinline__ bool chol_diag_body(double *S, int ld, int kb, double *Linv, int *flag, int store_L, int nact, [[maybe_unused]] int tl)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double *L = reinterpret_cast<double *>(smem_raw);  // [128][DL]
    if (threadIdx.x >= 64) __builtin_amdgcn_s_setprio(2);   // wave 0 carries the serial chain: its few MFMAs go before its SIMD neighbour's
    __shared__ double rd[NB + 2];                       // L's diagonal (the leaves hold their inverse in place); [NB] = breakdown flag
    double *misc = rd + NB;                             // (16-byte multiple keeps the dynamic base aligned)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    double *A = S + ((size_t)kb * NB) * ld + (size_t)kb * NB;
    if (t == 0) misc[0] = 0.0;
    {   // the block, 128 KB, as 16-byte loads ALL in flight before the first is used (round 2 loaded element by element
        // with 256 threads: ~25 us of this kernel's 83 were this loop)
        constexpr int PER = NB * (NB / 2) / (64 * CDW);      // 16-byte chunks per thread
        f64x2 v[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = t + 64 * CDW * q, r = i / (NB / 2), c2 = i % (NB / 2);
            v[q] = *reinterpret_cast<const f64x2 *>(A + (size_t)r * ld + 2 * c2);
        }
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = t + 64 * CDW * q, r = i / (NB / 2), c = 2 * (i % (NB / 2));
            L[r * DL + c] = c <= r ? v[q][0] : 0.0;
            L[r * DL + c + 1] = c + 1 <= r ? v[q][1] : 0.0;
        }
    }
    __syncthreads();
    STAMP(0);
    // 1a. 16x16 leaf by wave 0 alone, on the matrix pipe.  The block lives in ONE accumulator tile S (all 256 entries,
    //     kept symmetric) and is eliminated four columns at a time:
    //       - the 4x4 diagonal block is pulled into wave-uniform values (v_readlane) and factored AND inverted there,
    //         ~60 scalar-shaped f64 operations; M = (its factor)^-1, padded with zeros, becomes an MFMA A operand;
    //       - M x S[p] gives the four columns of L for ALL sixteen rows at once, already in operand layout
    //         (lane (row, k)), and S -= P P^T is one more MFMA;
    //       - the identity, carried along as extra rows (T2 = its transpose), undergoes the same column operations and
    //         ends as L^-T: the leaf inverse costs two more MFMAs per step instead of a 136-term substitution.
    //     Entries of S and T2 left of the active columns turn into rounding residue and are never read for a stored
    //     value.  (Round 2's leaf kept one row per lane and did all of this on the vector ALU: ~1200 instructions and
    //     8.6k cycles per leaf, the longest serial stretch of the factorisation's critical chain.)
    double *out = Linv + (size_t)kb * NB * NB;
    unsigned mk[10];      // slot of M[i][k] (i >= k, row-major over the lower triangle) -> all-ones in the lane (i, k) that holds it
    {
        const int c = lane & 15, g = lane >> 4;
#pragma unroll
        for (int i = 0, slot = 0; i < 4; ++i)
#pragma unroll
            for (int k = 0; k <= i; ++k, ++slot) mk[slot] = (c == i && g == k) ? 0xFFFFFFFFu : 0u;
    }
    auto leaf_factor = [&](int c0) {
            double *Lb = L + c0 * DL + c0;
            const int c = lane & 15, g = lane >> 4;
            f64x4 Sm, T2;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = g + 4 * r;
                Sm[r] = Lb[(i > c ? i : c) * DL + (i > c ? c : i)];
                T2[r] = i == c ? 1.0 : 0.0;
            }
            double Lc[4], Yc[4];
            double last = 0.0;
            const f64x4 zero4 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                auto pick = [&](int k, int j) {      // S[4p+k][4p+j] as a uniform value
                    const int src = 4 * p + j + 16 * k;
                    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(Sm[p]), src),
                                            __builtin_amdgcn_readlane(__double2loint(Sm[p]), src));
                };
                // 1/sqrt(d): v_rsq_f64 is good to 2^-24 (measured over 2^26 arguments), one cubic step
                // y (1 + e/2 + 3 e^2/8), e = 1 - d y^2, leaves |1 - d y^2| <= 2.8e-16 in four dependent operations.
                // A pivot that is not positive and finite makes y a NaN, and the NaN reaches every later pivot.
                auto rsq3 = [&](double d) {
                    const double y = __builtin_amdgcn_rsq(d);
                    const double e = fma(-(d * y), y, 1.0);
                    return fma(y * e, fma(0.375, e, 0.5), y);
                };
                // the A operand of the solve, lane (i = c, k = g) = M[i][k], assembled by mask as each value appears
                // (selects here turn into divergent branches around the scalar chain)
                unsigned mlo = 0, mhi = 0;
                auto put = [&](double v, int slot) { mlo |= (unsigned)__double2loint(v) & mk[slot]; mhi |= (unsigned)__double2hiint(v) & mk[slot]; };
                double d00 = pick(0, 0), d10 = pick(1, 0), d20 = pick(2, 0), d30 = pick(3, 0), d11 = pick(1, 1),
                       d21 = pick(2, 1), d31 = pick(3, 1), d22 = pick(2, 2), d32 = pick(3, 2), d33 = pick(3, 3);
                const double i0 = rsq3(d00);
                put(i0, 0);
                const double l10 = d10 * i0, l20 = d20 * i0, l30 = d30 * i0;
                d11 = fma(-l10, l10, d11); d21 = fma(-l20, l10, d21); d31 = fma(-l30, l10, d31);
                d22 = fma(-l20, l20, d22); d32 = fma(-l30, l20, d32); d33 = fma(-l30, l30, d33);
                const double i1 = rsq3(d11);
                put(i1, 2);
                const double m10 = -i1 * (l10 * i0);
                put(m10, 1);
                const double l21 = d21 * i1, l31 = d31 * i1;
                d22 = fma(-l21, l21, d22); d32 = fma(-l31, l21, d32); d33 = fma(-l31, l31, d33);
                const double i2 = rsq3(d22);
                put(i2, 5);
                const double m21 = -i2 * (l21 * i1), m20 = -i2 * fma(l21, m10, l20 * i0);
                put(m21, 4); put(m20, 3);
                const double l32 = d32 * i2;
                d33 = fma(-l32, l32, d33);
                const double i3 = rsq3(d33);
                const double m32 = -i3 * (l32 * i2), m31 = -i3 * fma(l32, m21, l31 * i1);
                const double m30 = -i3 * fma(l32, m20, fma(l31, m10, l30 * i0));
                put(i3, 9); put(m32, 8); put(m31, 7); put(m30, 6);
                last = i3;
                const double mop = __hiloint2double((int)mhi, (int)mlo);
                const f64x4 X = __builtin_amdgcn_mfma_f64_16x16x4f64(mop, Sm[p], zero4, 0, 0, 0);   // [0]: lane (j, g) = L[j][4p+g]
                if (p < 3) Sm = __builtin_amdgcn_mfma_f64_16x16x4f64(-X[0], X[0], Sm, 0, 0, 0);
                const f64x4 Y = __builtin_amdgcn_mfma_f64_16x16x4f64(mop, T2[p], zero4, 0, 0, 0);   // [0]: lane (e, g) = L^-T[e][4p+g]
                if (p < 3) T2 = __builtin_amdgcn_mfma_f64_16x16x4f64(-X[0], Y[0], T2, 0, 0, 0);
                Lc[p] = X[0]; Yc[p] = Y[0];
            }
            const bool ok = isfinite(last);
            if (!ok && lane == 0) misc[0] = 1.0;
            // lane (c, g), m = 4p + g: the INVERSE goes in place (entry [m][c], m >= c) -- every later reader of this block
            // (the solves below, the doubling steps, the output) wants the inverse; the factor itself is only ever stored
            // on request and waits transposed above the diagonal ([m][c] = L[c][m], m < c), its diagonal in rd
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int m = 4 * p + g;
                Lb[m * DL + c] = m >= c ? Yc[p] : Lc[p];
                if (m == c) rd[c0 + c] = Lc[p];
            }
            };
    const int NA = LB * ((min(max(nact, 1), NB) + LB - 1) / LB);      // rows of the leaves that hold active rows (a multiple of 16, at least one leaf)
    if (w == 0) leaf_factor(0);
    // the padding: unit diagonal of the factor (rd: what store_L reads) and of the inverse; everything else there is zero already --
    // the block was loaded with zeros above the diagonal, the padding rows are zero left of it, and the inverse's buffer starts as zeros
    for (int i = NA + t; i < NB; i += 64 * CDW) { rd[i] = 1.0; out[(size_t)i * NB + i] = 1.0; }
    __syncthreads();
    STAMP(1);
    f64x4 tcur = {0.0, 0.0, 0.0, 0.0};       // waves 1..7: T_j of the inverse's next block row (2., below)
    for (int c0 = 0; c0 < NA; c0 += LB) {
        if (misc[0] != 0.0) {
            if (t == 0) flag_raise(flag, 1);
            return false;
        }
        const int r0 = c0 + LB, kk = c0 / LB;
        if (r0 >= NA) break;
        // 1b. rows below: X = A * D^-T as 16x16 MFMA tiles (one wave per tile), in place:
        //     X[r][c] = sum_{k<=c} A[r][k] * Dinv[c][k]
        {
            const int leaf = c0 / LB, ntile = (NA - r0) / 16;
            for (int tile = w; tile < ntile; tile += CDW) {
                double *At = L + (r0 + 16 * tile) * DL + c0;
                f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < LB; kk += 4) {
                    const int k = kk + (lane >> 4), c = lane & 15;
                    const double a = At[(lane & 15) * DL + k];
                    const double b = k <= c ? L[(LB * leaf + c) * DL + LB * leaf + k] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) At[((lane >> 4) + 4 * reg) * DL + (lane & 15)] = acc[reg];
            }
        }
        __syncthreads();
        STAMP(32 + 2 * (c0 / LB));
        // 1c. trailing square -= panel panel^T, lower 16x16 tiles on MFMA: the accumulator starts
        //     as the C tile and the A operand is negated.  LOOKAHEAD: wave 0 takes tile (0,0) -- the next
        //     leaf's diagonal block -- and goes straight on to factor and invert that leaf while waves
        //     1..3 update the rest of the square, so the serial leaf work hides behind the MFMA work.
        {
            const int nt = (NA - r0) / 16, ntile = nt * (nt + 1) / 2;
            for (int tile = w == 0 ? 0 : w; tile < ntile; tile += (w == 0 ? ntile : CDW - 1)) {
                int tr = (int)((sqrtf(8.f * tile + 1.f) - 1.f) * 0.5f);
                while ((tr + 1) * (tr + 2) / 2 <= tile) ++tr;
                while (tr * (tr + 1) / 2 > tile) --tr;
                const int tcn = tile - tr * (tr + 1) / 2;
                double *Ct = L + (r0 + 16 * tr) * DL + r0 + 16 * tcn;
                const double *Pa = L + (r0 + 16 * tr) * DL + c0, *Pb = L + (r0 + 16 * tcn) * DL + c0;
                f64x4 acc;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) acc[reg] = Ct[((lane >> 4) + 4 * reg) * DL + (lane & 15)];
#pragma unroll
                for (int kk = 0; kk < LB; kk += 4) {
                    const int k = kk + (lane >> 4);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-Pa[(lane & 15) * DL + k], Pb[(lane & 15) * DL + k], acc, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) Ct[((lane >> 4) + 4 * reg) * DL + (lane & 15)] = acc[reg];
            }
            if (w == 0) leaf_factor(r0);
            else if (w - 1 <= kk) {
                // 2. the inverse grows a block row per leaf, behind the leaf work of wave 0:  Linv[k][j] = -Dinv_k T_j  with
                //    T_j = sum_{m = j .. k-1} L[k][m] Linv[m][j].  Wave j + 1 owns tile column j for good: it finishes row kk
                //    (T_j came with it from the last step, in registers: accumulator layout IS the B-operand layout),
                //    keeps the block in the mirror position above the diagonal for its own later use, sends it to HBM, and
                //    builds T_j of row kk + 1 -- whose leaf wave 0 is factoring right now.  Every block it reads is its own
                //    or a finished leaf's, so there is no synchronisation beyond the barriers of the factorisation.
                const int j = w - 1, ci = lane & 15, kq = lane >> 4;
                f64x4 R = {0.0, 0.0, 0.0, 0.0};
                if (j < kk) {
#pragma unroll
                    for (int sx = 0; sx < 4; ++sx) {
                        const int k = 4 * sx + kq;
                        const double a = k <= ci ? -L[(c0 + ci) * DL + c0 + k] : 0.0;
                        R = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tcur[sx], R, 0, 0, 0);
                    }
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        L[(LB * j + kq + 4 * reg) * DL + c0 + ci] = R[reg];
                        out[(size_t)(c0 + kq + 4 * reg) * NB + LB * j + ci] = R[reg];
                    }
                }
                f64x4 T = {0.0, 0.0, 0.0, 0.0};
                const double *Ar = L + (r0 + ci) * DL;          // row of L[kk + 1][.] this lane feeds as A operand
                {   // m = j: the leaf inverse on the diagonal (lower triangular; above it sits the factor, transposed).  The wave
                    // that starts a tile column (j == kk) is the first to read that leaf's inverse: it also sends it to HBM.
#pragma unroll
                    for (int sx = 0; sx < 4; ++sx) {
                        const int k = 4 * sx + kq;
                        const double b = ci <= k ? L[(LB * j + k) * DL + LB * j + ci] : 0.0;
                        if (j == kk && ci <= k) out[(size_t)(c0 + k) * NB + c0 + ci] = b;
                        T = __builtin_amdgcn_mfma_f64_16x16x4f64(Ar[LB * j + k], b, T, 0, 0, 0);
                    }
                }
                if (j + 1 < kk) {    // the blocks between, operands of step m + 1 requested before the MFMAs of step m
                    double an[4], bn[4];
#pragma unroll
                    for (int sx = 0; sx < 4; ++sx) { an[sx] = Ar[LB * (j + 1) + 4 * sx + kq]; bn[sx] = L[(LB * j + 4 * sx + kq) * DL + LB * (j + 1) + ci]; }
                    for (int m = j + 1; m < kk; ++m) {
                        double ac[4], bc[4];
#pragma unroll
                        for (int sx = 0; sx < 4; ++sx) { ac[sx] = an[sx]; bc[sx] = bn[sx]; }
                        const int mn = m + 1 < kk ? m + 1 : m;
#pragma unroll
                        for (int sx = 0; sx < 4; ++sx) { an[sx] = Ar[LB * mn + 4 * sx + kq]; bn[sx] = L[(LB * j + 4 * sx + kq) * DL + LB * mn + ci]; }
#pragma unroll
                        for (int sx = 0; sx < 4; ++sx) T = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[sx], bc[sx], T, 0, 0, 0);
                    }
                }
                if (j < kk) {
#pragma unroll
                    for (int sx = 0; sx < 4; ++sx) T = __builtin_amdgcn_mfma_f64_16x16x4f64(Ar[c0 + 4 * sx + kq], R[sx], T, 0, 0, 0);
                }
                tcur = T;
            }
        }
        __syncthreads();
        STAMP(33 + 2 * (c0 / LB));
    }
    STAMP(13);
    // The factor of the diagonal tile itself is read by nobody (panels and triangular solves use its
    // inverse) except for the right-hand-side row inside the LAST tile (k_ba_y_from_row): stored on request.
    if (store_L)
        for (int i = t; i < NB * NB; i += 64 * CDW) {
            const int r = i / NB, c = i % NB;
            if (c <= r) A[(size_t)r * ld + c] = r / LB != c / LB ? L[r * DL + c] : r == c ? rd[r] : L[c * DL + r];
        }
    STAMP(14);
    // the last ACTIVE block row of the inverse: its leaf was the last thing the loop did (tile columns left of it only: with one
    // active leaf there are none)
    if (w >= 1) {
        const int j = w - 1, c0 = NA - LB, ci = lane & 15, kq = lane >> 4;
        f64x4 R = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int sx = 0; sx < 4; ++sx) {
            const int k = 4 * sx + kq;
            const double a = k <= ci ? -L[(c0 + ci) * DL + c0 + k] : 0.0;
            R = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tcur[sx], R, 0, 0, 0);
        }
        if (LB * j < c0)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) out[(size_t)(c0 + kq + 4 * reg) * NB + LB * j + ci] = R[reg];
        if (w == 1) {
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                const int k = 4 * sx + kq;
                if (ci <= k) out[(size_t)(c0 + k) * NB + c0 + ci] = L[(c0 + k) * DL + c0 + ci];
            }
        }
    }
    STAMP(16);
    STAMP(17);
    TL_MARK(tl, 2);
    return true;
}
// (x_out != nullptr, systems of ONE block -- the reference's own sizes up to a dozen cameras; round 5: the backward substitution of the
//  block rides in this launch, x = Linv' y with y = row `yrow` of the factor just stored.  The arithmetic is k_trsv_bwd_chain's for its
//  last block row -- four partial sums of 32, combined pairwise -- so the bits are the same; one launch less per LM iteration.)
__global__ __launch_bounds__(64 * CDW) void k_chol_diag(double *S, int ld, int kb, double *Linv, int *flag, int store_L, Gate g, int nact = NB, int tl = 0,
                                                        double *x_out = nullptr, int yrow = 0)
{
    __builtin_amdgcn_s_setprio(3);
    TL_MARK(tl, 0);
    gate_enter(g);
    TL_MARK(tl, 1);
    const bool ok = chol_diag_body(S, ld, kb, Linv, flag, store_L, nact, tl);
    if (!x_out || !ok) return;              // (uniform)
    static_assert(64 * CDW == 512, "the substitution's four groups of 128 threads");
    __shared__ double xk[NB], part[4][NB];
    __syncthreads();                         // the block's inverse and its last row are in memory for every thread of the workgroup
    const int t = threadIdx.x & 127, gq = threadIdx.x >> 7;
    const double *Lk = Linv + (size_t)kb * NB * NB;
    double li[32];
#pragma unroll
    for (int m = 0; m < 32; ++m) li[m] = Lk[(size_t)(32 * gq + m) * NB + t];
    if (gq == 0) {
        const int idx = kb * NB + t;
        xk[t] = idx < yrow ? S[(size_t)yrow * ld + idx] : 0.0;
    }
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int m = 0; m < 32; ++m) sum += li[m] * xk[32 * gq + m];      // zeros above the diagonal
    part[gq][t] = sum;
    __syncthreads();
    if (gq == 0) x_out[(size_t)kb * NB + t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
}
// The diagonal blocks of a whole factorisation in ONE workgroup that stays resident (round 5).  As a launch per block the 512-thread,
// 132-KB workgroup had to find a CU every step -- and where the panel stream's latency kernels, unmasked since this round, fill the
// CUs that are kept free of bulk work, it waited ~50 us for one at every second step of the right-looking regime (device timeline).
// Here the workgroup keeps its CU: per block it waits for the counters the plan names (thread 0 polls, one agent-scope acquire,
// workgroup barrier -- the consumer recipe), factors the block exactly as k_chol_diag does, drains its stores, and publishes its
// ticket with an agent-scope release (a kernel boundary did that before).  A raised flag (breakdown: 1, a wait that timed out: 3)
// ends the loop; the host then does what it always did.
struct DiagItem { int kb, store_L, ticket, tl, nw, ctr[6], val[6]; };
__global__ __launch_bounds__(64 * CDW) void k_chol_diag_server(double *S, int ld, double *Linv, int *flag, const DiagItem *__restrict__ items, int n_items, int *ctr_base, int own_ctr,
                                                                int n_active)
{
    __builtin_amdgcn_s_setprio(3);
    __shared__ int s_stop;
    for (int it = 0; it < n_items; ++it) {
        const DiagItem item = items[it];
        TL_MARK(item.tl, 0);
        if (threadIdx.x == 0) {
            for (int i = 0; i < 6; ++i)
                if (i < item.nw) ring_wait(ctr_base + item.ctr[i], item.val[i], flag);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_stop = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        }
        __syncthreads();
        if (s_stop) return;
        TL_MARK(item.tl, 1);
        const int nact = min(NB, n_active - item.kb * NB);
        const bool ok = chol_diag_body(S, ld, item.kb, Linv, flag, item.store_L, nact, item.tl);
        if (!ok) return;                        // (uniform: every thread read the same LDS word behind a barrier)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(ctr_base + own_ctr, item.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Dense blocked Cholesky, GEMM side.  S holds the reduced system and its trailing updates; the
// panels  P[i,kb] = S[i,kb] Linv_kb^T  (the sub-diagonal tiles of L) are written to a separate
// matrix L, so no kernel ever overwrites an operand another workgroup is still reading.
//
// k_gemm_q<0> (panel)  and  k_gemm_q<1> (first trailing tile column: S[i,kb+1] -= L[i,kb] L[kb+1,kb]^T)
// are the serial chain the next diagonal block waits for, so they are built for latency and for
// running BESIDE the bulk update, whose two resident workgroups per CU hold 128 KB of LDS and
// ~420 of the 512 VGPRs of a SIMD: no LDS, no barrier, at most 96 VGPRs.  One wave owns one 16x16
// output tile (a 128x128 tile = 64 waves) and loads its operands straight into MFMA layout, K in
// two halves of 64: per half 8 + 8 sixteen-byte loads per lane (lane group fk takes k = 8 g + 2 fk
// and + 1 of every 8-wide group g, so a load instruction covers 16 rows x one 64-B line), then 16
// v_mfma_f64_16x16x4_f64.  The four workgroups that share a 32-row A strip carry the same
// (blockIdx & 7), i.e. run on the same XCD and share the strip in its L2.
// k_gemm_nt_pipe (the rest of the trailing update, S[i,j] -= L[i,kb] L[j,kb]^T for kb+1 < j <= i)
// runs beside them on its own stream and is built for throughput.
// first / m: the tiles kb + 1 + first .. kb + 1 + first + m - 1 of the tile column (the critical tile is first = 0, m = 1)
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(96)))
void k_gemm_q(double *S, double *L, int ld, int kb, int first, int m, const double *Linv, Gate g, int dj = 1, int tl = 0)
{
    __builtin_amdgcn_s_setprio(3);      // these waves share SIMDs with the bulk update's: their few MFMAs and loads go first
    [[maybe_unused]] const int tl_id = tl;
    TL_MARK(tl_id, 0);
    gate_enter(g);
    TL_MARK(tl_id, 1);
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int strip = 8 * (slot >> 2) + xcd, qj = slot & 3;      // strip: 32 rows of the tile column, qj: 32 output columns
    if (strip >= 4 * m) return;
    const int tj = MODE == 0 ? kb : kb + dj;      // MODE 1: the tile column that is updated, S(i, kb + dj) -= L(i, kb) L(kb + dj, kb)'
    const size_t row0 = (size_t)(kb + 1 + first) * NB + 32 * (size_t)strip;
    const double *A = (MODE == 0 ? S : L) + row0 * ld + (size_t)kb * NB;
    const double *B = MODE == 0 ? Linv + (size_t)kb * NB * NB + (size_t)(32 * qj) * NB
                                : L + ((size_t)tj * NB + 32 * qj) * ld + (size_t)kb * NB;
    const int ldb = MODE == 0 ? NB : ld;
    double *C = (MODE == 0 ? L : S) + row0 * ld + (size_t)tj * NB + 32 * qj;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = (w >> 1) * 16, wc = (w & 1) * 16;
    const int fr = lane & 15, fk = lane >> 4;
    const f64x2 *ap = reinterpret_cast<const f64x2 *>(A + (size_t)(wr + fr) * ld + 2 * fk);
    const f64x2 *bp = reinterpret_cast<const f64x2 *>(B + (size_t)(wc + fr) * ldb + 2 * fk);
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg.  The accumulators start as the
    // C tile and the A operand is negated, so C - A B^T comes straight out of the MFMA chain.
    f64x4 acc;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) acc[reg] = MODE == 0 ? 0.0 : C[(size_t)(wr + fk + 4 * reg) * ld + wc + fr];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f64x2 a[8], b[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) { a[g] = ap[4 * (8 * half + g)]; b[g] = bp[4 * (8 * half + g)]; }
#pragma unroll
        for (int g = 0; g < 8; ++g)
#pragma unroll
            for (int h = 0; h < 2; ++h)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(MODE == 0 ? a[g][h] : -a[g][h], b[g][h], acc, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) C[(size_t)(wr + fk + 4 * reg) * ld + wc + fr] = acc[reg];
    TL_MARK(tl_id, 2);
}

// The same latency form for the two-level regime's head (round 5): a LIST of tiles (map entry: row << 16 | column), several panels
// per tile, the accumulators kept in registers across them --
//   MODE 1  S(i, j) -= sum_q L(i, kb + q) L(j, kb + q)'              q < npan: the next super-diagonal block, K = 128 g
//   MODE 2  L(i, kb + c) = sum_{m <= c} S(i, kb + m) W[c][m]'         c = the entry's column: the head rows' panel product
// As pipelined launches (one 128 x 128 tile per workgroup, K = 512: 64 stages) these two sat on the chain's critical path for
// ~70 us each alone and ~100 us beside the bulk update; here a tile is 32 workgroups of four 16 x 16 waves, operands straight
// from L2 into MFMA layout, no LDS, at most 96 registers -- they fit beside anything.  Workgroup b: tile b / 16, a 32 x 32 part of it.
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_num_vgpr(96)))
void k_gemm_qm(double *S, double *L, int ld, int kb, const unsigned *__restrict__ map, int npan, const double *SI, int ldsi, Gate g, int tl)
{
    static_assert(MODE == 1 || MODE == 2, "update / panel product");
    __builtin_amdgcn_s_setprio(3);
    TL_MARK(tl, 0);
    gate_enter(g);
    TL_MARK(tl, 1);
    const unsigned e = map[blockIdx.x >> 4];
    if (e == ~0u) return;
    const int ti = (int)(e >> 16), ecol = (int)(e & 0x3fffu);
    const int sub = blockIdx.x & 15, strip = sub >> 2, qj = sub & 3;      // strip: 32 rows of the tile, qj: 32 output columns
    const int tj = MODE == 1 ? ecol : kb + ecol;
    const int np = MODE == 1 ? npan : ecol + 1;
    const size_t row0 = (size_t)ti * NB + 32 * (size_t)strip;
    const double *A = (MODE == 1 ? L : S) + row0 * ld + (size_t)kb * NB;
    const double *B = MODE == 1 ? L + ((size_t)tj * NB + 32 * qj) * ld + (size_t)kb * NB : SI + ((size_t)ecol * NB + 32 * qj) * ldsi;
    const int ldb = MODE == 1 ? ld : ldsi;
    double *C = (MODE == 1 ? S : L) + row0 * ld + (size_t)tj * NB + 32 * qj;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int wr = (w >> 1) * 16, wc = (w & 1) * 16;
    const int fr = lane & 15, fk = lane >> 4;
    const f64x2 *ap = reinterpret_cast<const f64x2 *>(A + (size_t)(wr + fr) * ld + 2 * fk);
    const f64x2 *bp = reinterpret_cast<const f64x2 *>(B + (size_t)(wc + fr) * ldb + 2 * fk);
    f64x4 acc;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) acc[reg] = MODE == 2 ? 0.0 : C[(size_t)(wr + fk + 4 * reg) * ld + wc + fr];
    for (int q = 0; q < np; ++q) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f64x2 a[8], b[8];
#pragma unroll
            for (int gq = 0; gq < 8; ++gq) { a[gq] = ap[64 * q + 4 * (8 * half + gq)]; b[gq] = bp[64 * q + 4 * (8 * half + gq)]; }
#pragma unroll
            for (int gq = 0; gq < 8; ++gq)
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(MODE == 2 ? a[gq][h] : -a[gq][h], b[gq][h], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) C[(size_t)(wr + fk + 4 * reg) * ld + wc + fr] = acc[reg];
    TL_MARK(tl, 2);
}

// Two-level regime (round 5): block row `pos` of W = L_JJ^-1, the inverse of the factor of the super-diagonal block [p, p + g) --
// g x g tiles, lower block-triangular, row-major in SI (row stride ldsi = 128 g):
//     W[pos][pos] = Linv_c,     W[pos][m] = -Linv_c  sum_{r = m .. pos-1} L(c, p + r) W[r][m]     (c = p + pos, m < pos)
// from L W = I.  With it every row below the super-block is ONE product, L(i, J) = S(i, J) W' (k_gemm_nt_pipe, MODE 2), instead
// of g panel products with g (g - 1) / 2 column updates between them.  Workgroup b < 8 pos: tile m = b / 8, its 16-column strip
// b % 8 -- eight waves, wave w the strip's rows 16 w .. 16 w + 15: first the sum (operands straight from L2 into MFMA layout,
// both fed with the same k permutation), through LDS, then the product with Linv_c, whose rows 16 w .. end at column 16 w + 15.
// The last workgroup copies the diagonal tile.  A few microseconds behind the chain's next diagonal block; only the last row
// of a super-block is waited for.
__global__ __launch_bounds__(512) void k_sinv(const double *L, int ld, const double *Linv, double *SI, int ldsi, int p, int pos, Gate g, int tl)
{
    __builtin_amdgcn_s_setprio(3);
    TL_MARK(tl, 0);
    gate_enter(g);
    TL_MARK(tl, 1);
    const int c = p + pos, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const double *Lc = Linv + (size_t)c * NB * NB;
    if ((int)blockIdx.x == 8 * pos) {
        for (int i = t; i < NB * NB / 2; i += 512) {
            const int r = i / (NB / 2), c2 = i % (NB / 2);
            *reinterpret_cast<f64x2 *>(SI + ((size_t)pos * NB + r) * ldsi + (size_t)pos * NB + 2 * c2) = *reinterpret_cast<const f64x2 *>(Lc + (size_t)r * NB + 2 * c2);
        }
        TL_MARK(tl, 2);
        return;
    }
    const int m = blockIdx.x >> 3, strip = blockIdx.x & 7;
    __shared__ double Y[NB][17];
    const int fr = lane & 15, fk = lane >> 4;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int r = m; r < pos; ++r) {
        const double *A = L + ((size_t)c * NB + 16 * w + fr) * ld + (size_t)(p + r) * NB + 2 * fk;
        const double *B = SI + ((size_t)r * NB + 2 * fk) * ldsi + (size_t)m * NB + 16 * strip + fr;
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            f64x2 a[8];
            double b0[8], b1[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int k0 = 64 * half + 8 * q;
                a[q] = *reinterpret_cast<const f64x2 *>(A + k0);
                b0[q] = B[(size_t)k0 * ldsi];
                b1[q] = B[(size_t)(k0 + 1) * ldsi];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][0], b0[q], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][1], b1[q], acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) Y[16 * w + fk + 4 * reg][fr] = acc[reg];
    __syncthreads();
    f64x4 o = {0.0, 0.0, 0.0, 0.0};
    const double *Ar = Lc + (size_t)(16 * w + fr) * NB + 2 * fk;
    for (int k0 = 0; k0 < 16 * (w + 1); k0 += 8) {
        const f64x2 a = *reinterpret_cast<const f64x2 *>(Ar + k0);
        o = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[0], Y[k0 + 2 * fk][fr], o, 0, 0, 0);
        o = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[1], Y[k0 + 2 * fk + 1][fr], o, 0, 0, 0);
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) SI[((size_t)pos * NB + 16 * w + fk + 4 * reg) * ldsi + (size_t)m * NB + 16 * strip + fr] = o[reg];
    TL_MARK(tl, 2);
}

// Bulk trailing update, LDS-DMA ring:  S[i,j] -= L[i, kb..] L[j, kb..]^T  over 8-wide k-stages.  Operands reach LDS by LDS-DMA only -- no staging registers --
// through a 4-stage ring, three stages (24 k) ahead of the MFMAs, behind counted vmcnt waits and one
// raw s_barrier per stage.  A stage holds, per operand, 128 rows x 8 doubles as eight 1-KiB
// row groups in PIECE-MAJOR order (slot = piece * 16 + row, 16 B per slot): each DMA lane picks
// the global 16 B that belongs in its linear LDS slot, so a ds_read_b128 of 16 rows x one piece
// is one whole 256-B bank row (conflict-free without padding) and yields the operands of two
// MFMA steps (lane group fk supplies k = 2 fk and 2 fk + 1).
#define GST 4
#define GSTAGE_BYTES (2 * 128 * 8 * 8)   // A + B, 16 KiB
// The bulk kernel (round 3; round 2's k_gemm_nt_ring, same tile, ring and operand layout, waited for LDS inside every stage and read its C tile up front).  What changed is
// where a wave waits.  Measured on the ring form (tools/gemm_nt_bench, tools/mfma_f64_peak): the bare
// v_mfma_f64_16x16x4_f64 loop sustains 77 TFLOP/s on this chip (64 cycles per MFMA at ~2.36 GHz: f64 is not
// clock-limited), the ring form's loop alone 58 (operands + barrier exposed once per 8-k stage) and a K = 128 pass 37:
// a third of a pass is the C tile -- 128 KB read into the accumulators BEFORE the first MFMA, 128 KB stored after the last.
//   * operand fragments are double-buffered in registers: the ds_read_b128s of stage s+1 are issued in front of the 32
//     MFMAs of stage s, so a wave never waits for LDS between two MFMA bursts (only for the stage barrier);
//   * the accumulators start at zero and the C tile is folded in ON THE WAY: the wave's sixteen 16x16 tiles of C are
//     requested two at a time at the even stages 0, 2, .. 14 and added to their accumulators one stage (~2500 cycles)
//     later -- no load of C is waited for, and what is left at the end is the store.  C moves through buffer
//     instructions (one descriptor in SGPRs, one per-lane offset, wave-uniform row / tile offsets as scalar offsets): with
//     128 accumulator and 64 operand registers per lane there is no room for per-tile 64-bit addresses.
// With the stage index known at compile time every wait count below is a literal and the loop has no branch.
#define PIPE_PRIO 0x200      // flag: raise the wave priority (launches on the panel stream: they share SIMDs with the bulk update)
// f(integral_constant<int, BASE + I>) for I = 0 .. : the stage loop with the stage number as a compile-time constant
template <int BASE, int... I, class F> __device__ __forceinline__ void pipe_for_seq(std::integer_sequence<int, I...>, F &&f)
{
    (f(std::integral_constant<int, BASE + I>{}), ...);
}
// Round 5.  Map entries name ABSOLUTE tiles: row << 16 | class << 14 | column (chol_plan.h); a tile of class 1 / 2 is counted out in
// sig[0] / sig[1] when it is finished (the tiles the next steps read first lead the launch).
// NST = 16 / 32: every stage at compile time (K = 128 / 256).  NST = 0: the ROLLED form for any longer pass -- sixteen compile-time
// stages that carry the C tiles, four-stage trips with running operand pointers, four compile-time stages at the end; the stage
// count is a run-time value, nst_rt (a multiple of 4, at least 24): one instance serves K = 512 and K = 1024 and the ragged
// passes of MODE 2.
// MODE 0  S(i, j) -= L(i, kb ..) L(j, kb ..)'          Out = S, Ain = L
// MODE 1  L(i, kb) = S(i, kb) Linv_kb'                 Out = L, Ain = S, Bm = Linv (row stride 128); no C tile
// MODE 2  L(i, kb + c) = S(i, kb .. kb + c) W[c][.]'    Out = L, Ain = S, Bm = the super-block's inverse W (row stride ldb_arg),
//         c = the entry's column: a pass of 16 (c + 1) stages; no C tile (the two-level regime's panel product)
//         (column 0 as 24 stages, K = 192: the rolled form's shortest pass -- the 64 extra columns meet the zero block W[0][1])
template <int DBG, int NST, int MODE>
__device__ __forceinline__ void pipe_body(double *Out, const double *Ain, int ld, int kb, const unsigned e, int flags, int *sig, const double *Bm, int ldb_arg, int nst_rt, int tl)
{
    constexpr bool rolled = NST == 0;
    constexpr int NSTC = rolled ? 64 : NST;      // what the compile-time stages see: in the rolled form the first sixteen are far from the end and the last four know their distance to it
    static_assert(rolled || (NST % 4 == 0 && NST >= 16 && NST <= 32), "C tiles are folded in during stages 0 .. 15");
    static_assert(MODE != 2 || rolled, "the panel product of the two-level regime has ragged pass lengths");
    extern __shared__ __attribute__((aligned(16))) char gsm[];
    if (flags & PIPE_PRIO) __builtin_amdgcn_s_setprio(2);
    [[maybe_unused]] const int tl_id = tl;
    TL_MARK(tl_id, 0);
    const int ti = (int)(e >> 16), ecol = (int)(e & 0x3fffu), cls = (int)((e >> 14) & 3u);
    const int tj = MODE == 0 ? ecol : MODE == 1 ? kb : kb + ecol;
    const int nst = __builtin_amdgcn_readfirstlane(rolled ? (MODE == 2 ? (ecol == 0 ? 24 : 16 * (ecol + 1)) : nst_rt) : NST);
    const double *A = Ain + ((size_t)ti * NB) * ld + (size_t)kb * NB;
    const double *B = MODE == 0 ? Ain + ((size_t)tj * NB) * ld + (size_t)kb * NB : MODE == 1 ? Bm + (size_t)kb * NB * NB : Bm + ((size_t)ecol * NB) * ldb_arg;
    const int ldb = MODE == 0 ? ld : MODE == 1 ? NB : ldb_arg;
    double *S = Out;
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);      // wave-uniform, and the compiler should know: everything derived
                                                               // from it (ring slots, C descriptor, tile offsets) lives in SGPRs
    const int wr = (w >> 1) * 64, wc = (w & 1) * 64;
    const int fr = lane & 15, fk = lane >> 4;
    // the wave's 64 x 64 part of the C tile through a buffer descriptor: per-lane byte offset of its corner element,
    // everything else (tile row / column, register row) is wave-uniform and travels as the scalar offset
    double *Cw = S + ((size_t)ti * NB + wr) * ld + (size_t)tj * NB + wc;
    const __amdgpu_buffer_rsrc_t crs = __builtin_amdgcn_make_buffer_rsrc(Cw, 0, (int)(64 * (size_t)ld * 8), 0x00020000);
    const int cvo = (int)(((size_t)fk * ld + fr) * 8);
    const int ld8 = ld * 8;        // one row of the system in bytes (the C part of a wave spans 64 rows: far below 2^31)
    f64x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
    const double *srcA = A + (size_t)(32 * w + fr) * ld + 2 * fk;      // (advanced by the rolled middle of a long pass)
    const double *srcB = B + (size_t)(32 * w + fr) * ldb + 2 * fk;
    // slot: ring slot of the stage (stage number mod GST); k0: its first column relative to where srcA / srcB point (the rolled
    // middle of a long pass advances the two pointers, so that the offset stays an immediate)
    auto issue = [&](int slot, int k0) {
        char *buf = gsm + slot * GSTAGE_BYTES + 2048 * w;
        if (DBG & 4) return;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcA + (size_t)(16 * q) * ld + k0),
                                             (__attribute__((address_space(3))) void *)(buf + 1024 * q), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcB + (size_t)(16 * q) * ldb + k0),
                                             (__attribute__((address_space(3))) void *)(buf + 8192 + 1024 * q), 16, 0, 0);
        }
    };
    const unsigned base = (unsigned)(size_t)(const __attribute__((address_space(3))) char *)gsm;
    const unsigned offA = base + (unsigned)((wr >> 4) * 1024 + fk * 256 + fr * 16);
    const unsigned offB = base + (unsigned)(8192 + (wc >> 4) * 1024 + fk * 256 + fr * 16);
    f64x2 ra[2][4], rb[2][4];
    // wait until at most n of this wave's vector-memory operations (LDS-DMA pieces and C loads, in issue order) are pending
    auto wait_vm = [&](int n) {
        switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 12: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
        case 16: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
        case 20: asm volatile("s_waitcnt vmcnt(20)" ::: "memory"); break;
        case 24: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;      // a count this list does not know: wait for everything
        }
    };
    // "=&v": an LDS read writes its destination when the data returns -- it must not share a register with an address
    auto read_stage = [&](int P, int slot) {      // slot: ring slot of the stage that is read (stage number mod GST)
        const unsigned so = (unsigned)(slot * GSTAGE_BYTES);
        asm volatile("ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:1024\n\tds_read_b128 %2, %8 offset:2048\n\tds_read_b128 %3, %8 offset:3072\n\t"
                     "ds_read_b128 %4, %9\n\tds_read_b128 %5, %9 offset:1024\n\tds_read_b128 %6, %9 offset:2048\n\tds_read_b128 %7, %9 offset:3072"
                     : "=&v"(ra[P][0]), "=&v"(ra[P][1]), "=&v"(ra[P][2]), "=&v"(ra[P][3]), "=&v"(rb[P][0]), "=&v"(rb[P][1]), "=&v"(rb[P][2]), "=&v"(rb[P][3])
                     : "v"(offA + so), "v"(offB + so) : "memory");
    };
    for (int s = 0; s < GST; ++s) issue(s, 8 * s);
    // Stage s sits in register buffer s & 1.  Per stage: make stage s + 1 visible (its DMA pieces have landed for every
    // wave) and refill the ring slot stage s has just left; fold C tile s in; request C tile s + 2; request the operands of
    // stage s + 1; the 32 MFMAs.  The sixteen 16x16 tiles of C are requested ONE at a time, tiles 0 and 1 behind the ring's
    // prologue and tile s + 2 at stage s, and folded in TWO stages after their request (round 3 requested two tiles at the
    // even stages and folded them one stage later: the same sixteen registers, half the time for the load -- and a stage
    // lasts ~1.9 us with two workgroups on the CU, which is what a read from HBM takes under load: the fold waited at every
    // odd stage).
    // Vector-memory operations of a wave in issue order:  D0 D1 D2 D3 C0 C1 | D4 C2 | D5 C3 | ... (D = 4 DMA pieces, C = 4 loads);
    // every wait below counts the operations YOUNGER than the one it needs, which may stay pending.
    typedef int v2i __attribute__((ext_vector_type(2)));
    v2i craw[2][4];
    constexpr int NCT = MODE == 0 ? 16 : 0;            // C tiles
    constexpr bool with_c = NCT > 0 && !(DBG & 1);
    auto c_req = [&](int tile) {
        // inline asm: a load the compiler issues itself it also waits for itself, with vmcnt(0) -- the counter is in-order and
        // it cannot tell the DMA pieces behind the load from the load -- which would drain the ring at every stage
        const int ci = tile >> 2, cj = tile & 3;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            asm volatile("buffer_load_dwordx2 %0, %1, %2, %3 offen" : "=&v"(craw[tile & 1][reg]) : "v"(cvo + 128 * cj), "s"(crs), "s"((16 * ci + 4 * reg) * ld8) : "memory");
    };
    auto fold = [&](int tile) {
        const int ci = tile >> 2, cj = tile & 3, B = tile & 1;
        asm volatile("" : "+v"(craw[B][0]), "+v"(craw[B][1]), "+v"(craw[B][2]), "+v"(craw[B][3]));
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            union { v2i r; double d; } u;
            u.r = craw[B][reg];
            acc[ci][cj][reg] -= u.d;          // the accumulators hold A B' - C: the sign turns at the store
        }
    };
    // C loads among the tiles lo .. hi (those that exist)
    auto n_c = [&](int lo, int hi) { int n = 0; for (int j = lo; j <= hi; ++j) n += (with_c && j >= 0 && j < NCT) ? 1 : 0; return n; };
    if (with_c) { c_req(0); c_req(1); }
    wait_vm(12 + 4 * n_c(0, 1));
    __builtin_amdgcn_s_barrier();
    read_stage(0, 0);
    // One stage.  SC >= 0: the stage number is a compile-time constant (the first sixteen stages, which carry the C tiles, and the
    // last four, whose waits shrink with the ring); SC < 0: a stage of the rolled middle of a long pass (K = 384, 512: round 4),
    // stage number s_rt at run time, parity PAR of its register buffer at compile time, every wait the steady-state literal.
    auto stage = [&](auto sc, auto pos, int s_rt) {
        constexpr int SC = decltype(sc)::value, POS = decltype(pos)::value, P = POS & 1;      // POS: stage number mod GST
        constexpr bool mid = SC < 0;
        const int s = mid ? s_rt : SC;
        // my reads of stage s (requested one stage ago) have returned: the fragments are in their registers and the ring
        // slot is free on my side.  The ONLY LDS wait of the step -- the reads of stage s + 1 requested below stay in flight
        // behind this step's MFMAs (a wait in front of the MFMAs would wait for them too: the counter is in-order)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra[P][0]), "+v"(ra[P][1]), "+v"(ra[P][2]), "+v"(ra[P][3]), "+v"(rb[P][0]), "+v"(rb[P][1]), "+v"(rb[P][2]), "+v"(rb[P][3]) :: "memory");
        if (mid || SC + 1 < NSTC) {
            // needs D(s+1).  Younger: D(s+2), D(s+3); the C loads issued behind D(s+1): C0, C1 behind the prologue (all of
            // D0 .. D3 precede them), C(t+2) behind D(t+4) at stage t, i.e. C(s-1) .. C(s+1) for s >= 3
            if constexpr (mid) wait_vm(8);
            else {
                constexpr int c_younger = SC + 1 <= 3 ? (with_c ? (SC + 2 < NCT ? SC + 2 : NCT) : 0) : (with_c ? ((SC - 1 < NCT) + (SC < NCT) + (SC + 1 < NCT)) : 0);
                wait_vm(4 * ((SC + 2 < NSTC) + (SC + 3 < NSTC)) + 4 * c_younger);
            }
            __builtin_amdgcn_s_barrier();
            if constexpr (mid) issue(POS, 8 * POS);                 // into the slot of stage s (the pointers stand at the loop trip's first stage + GST)
            else if constexpr (SC + GST < NSTC) issue(POS, 8 * (SC + GST));
        }
        if constexpr (!mid && with_c && SC < NCT) {
            // needs C(s), requested two stages ago (tiles 0, 1: behind the prologue).  Younger: C(s+1), and every D issued
            // behind C(s): D(s+3) and D(s+4) for s >= 2, D4 and D5 for s = 1, D4 for s = 0 -- those that exist
            constexpr int d_younger = SC >= 2 ? (SC + 3 < NSTC) + (SC + GST < NSTC) : (SC == 1 ? (4 < NSTC) + (5 < NSTC) : (4 < NSTC));
            wait_vm(4 * d_younger + 4 * (SC + 1 < NCT ? 1 : 0));
            fold(SC);
            if (SC + 2 < NCT) c_req(SC + 2);
        }
        if (mid || SC + 1 < NSTC) read_stage(1 - P, (POS + 1) % GST);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[P][i][h], rb[P][j][h], acc[i][j], 0, 0, 0);
    };
    using ic_m1 = std::integral_constant<int, -1>;
    static_assert(GST == 4, "the rolled middle advances one ring turn per trip");
    if constexpr (!rolled) {
        // every stage at compile time (K = 128, 256)
        pipe_for_seq<0>(std::make_integer_sequence<int, NST>{}, [&](auto sc) { stage(sc, std::integral_constant<int, decltype(sc)::value % GST>{}, 0); });
    } else {
        pipe_for_seq<0>(std::make_integer_sequence<int, 16>{}, [&](auto sc) { stage(sc, std::integral_constant<int, decltype(sc)::value % GST>{}, 0); });
        srcA += 8 * (16 + GST); srcB += 8 * (16 + GST);                 // stage 16 issues stage 20
        for (int s4 = 16; s4 < nst - 4; s4 += 4) {
            stage(ic_m1{}, std::integral_constant<int, 0>{}, s4); stage(ic_m1{}, std::integral_constant<int, 1>{}, s4 + 1);
            stage(ic_m1{}, std::integral_constant<int, 2>{}, s4 + 2); stage(ic_m1{}, std::integral_constant<int, 3>{}, s4 + 3);
            srcA += 8 * GST; srcB += 8 * GST;
        }
        pipe_for_seq<NSTC - 4>(std::make_integer_sequence<int, 4>{}, [&](auto sc) { stage(sc, std::integral_constant<int, decltype(sc)::value % GST>{}, 0); });
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (!(DBG & 2) || acc[i][j][reg] == 1.2345e300) {
                    union { v2i r; double d; } u;
                    u.d = MODE != 0 ? acc[i][j][reg] : -acc[i][j][reg];                  // C - A B'  (MODE 1, 2: A B')
                    __builtin_amdgcn_raw_buffer_store_b64(u.r, crs, cvo + 128 * j, (16 * i + 4 * reg) * ld8, 0);
                }
    // The tiles the next steps read first lead the launch and are counted out one by one (class 1 / 2 of the map entry): nobody
    // waits for a whole bulk update except through stream order.
    if (sig && cls) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (t == 0) __hip_atomic_fetch_add(sig + (cls - 1), 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#ifdef RCN_DIAG
        if (g_tl && t == 0) atomicMax(&g_tl[3 * tl_id + 1], (unsigned long long)wall_clock64());      // a head tile finished
#endif
    }
    TL_MARK(tl_id, 2);
}
template <int DBG, int NST, int MODE = 0>
__global__ __launch_bounds__(256, 2) void k_gemm_nt_pipe(double *Out, const double *Ain, int ld, int kb, const unsigned *__restrict__ map, int flags, int *sig,
                                                          const double *Bm = nullptr, int ldb_arg = 0, int nst_rt = 0, int tl = 0)
{
    const unsigned e = map[blockIdx.x];
    if (e == ~0u) return;
    pipe_body<DBG, NST, MODE>(Out, Ain, ld, kb, e, flags, sig, Bm, ldb_arg, nst_rt, tl);
}
// ONE launch, two kinds of tiles (round 5): the trailing update of super-step J (the first `split` workgroups: MODE 0, rolled) and,
// behind them, the panel product of super-step J + 1 for the rows below its head (MODE 2).  Measured in the device timeline: as a
// launch of its own on another stream that product ran 2-5 times longer beside the bulk update than alone, and the bulk update
// 15 % longer beside it (47 against 53-59 TFLOP/s); here its tiles start where the bulk update's last round leaves slots free --
// they fill the drain -- and the next bulk update follows in stream order, without a gate.
// What a tail tile needs was produced elsewhere: the panel columns it reads by THIS launch's class-2 tiles (they lead the launch, so
// they were dispatched long before a tail workgroup can become resident: the wait cannot hold up what it waits for), the
// super-block's inverse by the chain and its followers on the panel stream, which run a super-step ahead of the bulk stream.
// Thread 0 polls (relaxed, bounded: 2 s -> flag 3 -> the one-stream schedule), one agent-scope acquire, workgroup barrier.
__global__ __launch_bounds__(256, 2) void k_gemm_nt_pipe_tail(double *S, double *L, int ld, int kb0, int nst0, const unsigned *__restrict__ map0, int split, int flags0, int *sig, int tl0,
                                                               int kb2, const unsigned *__restrict__ map2, const double *SI, int ldsi, Gate g2, int tl2)
{
    if ((int)blockIdx.x < split) {
        const unsigned e = map0[blockIdx.x];
        if (e == ~0u) return;
        pipe_body<0, 0, 0>(S, L, ld, kb0, e, flags0, sig, nullptr, 0, nst0, tl0);
    } else {
        const unsigned e = map2[blockIdx.x - split];
        if (e == ~0u) return;
        if (threadIdx.x == 0) {
            for (int i = 0; i < 6; ++i)
                if (i < g2.nw) ring_wait(g2.c[i], g2.n[i], g2.flag);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
#ifdef RCN_DIAG
        if (g_tl && threadIdx.x == 0 && (int)blockIdx.x == split) atomicMax(&g_tl[3 * tl2 + 0], (unsigned long long)wall_clock64());
#endif
        pipe_body<0, 0, 2>(L, S, ld, kb2, e, 0, nullptr, SI, ldsi, 0, tl2);
    }
}

// forward substitution step kb: y_kb = Linv_kb b_kb ; b_i -= L[i,kb] y_kb for i > kb.
// every workgroup recomputes y_kb (16k fma) and updates one 128-row tile.
__global__ __launch_bounds__(128) void k_trsv_fwd(const double *S /* = L: sub-diagonal tiles */, int ld, int kb, const double *Linv, double *b, double *y)
{
    __shared__ double yk[NB], bk[NB];
    const int t = threadIdx.x, i = kb + blockIdx.x;
    bk[t] = b[(size_t)kb * NB + t];
    __syncthreads();
    const double *Li = Linv + (size_t)kb * NB * NB + (size_t)t * NB;
    double s = 0.0;
#pragma unroll 8
    for (int m = 0; m < NB; ++m) s += (m <= t ? Li[m] : 0.0) * bk[m];   // Linv is stored with zeros above the diagonal
    yk[t] = s;
    __syncthreads();
    if (i == kb) { y[(size_t)kb * NB + t] = s; return; }
    const double *row = S + ((size_t)i * NB + t) * ld + (size_t)kb * NB;
    double u = 0.0;
#pragma unroll 16
    for (int m = 0; m < NB; ++m) u += row[m] * yk[m];
    b[(size_t)i * NB + t] -= u;
}

// backward substitution step kb (descending): x_kb = Linv_kb^T y_kb ; y_j -= L[kb,j]^T x_kb for j < kb
// 512 threads per workgroup: four groups of 128 split the 128 rows of each dot product (the 79 launches of a cfg-5
// solve are a serial chain: 12.5 us each with one thread per column walking all 128 rows, ~1 ms per LM iteration)
__global__ __launch_bounds__(512) void k_trsv_bwd(const double *S /* = L: sub-diagonal tiles */, int ld, int kb, const double *Linv, double *y, double *x)
{
    __shared__ double xk[NB], yk[NB], part[4][NB];
    const int t = threadIdx.x & 127, g = threadIdx.x >> 7, j = blockIdx.x;  // j = 0..kb ; j == kb writes x
    if (g == 0) yk[t] = y[(size_t)kb * NB + t];
    __syncthreads();
    const double *Lk = Linv + (size_t)kb * NB * NB;
    double s = 0.0;
#pragma unroll 8
    for (int m = 32 * g; m < 32 * g + 32; ++m) s += Lk[(size_t)m * NB + t] * yk[m];   // zeros above the diagonal
    part[g][t] = s;
    __syncthreads();
    if (g == 0) xk[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    __syncthreads();
    if (j == kb) { if (g == 0) x[(size_t)kb * NB + t] = xk[t]; return; }
    const double *blk = S + ((size_t)kb * NB) * ld + (size_t)j * NB;  // L[kb, j] tile, rows m, col t
    double u = 0.0;
#pragma unroll 8
    for (int m = 32 * g; m < 32 * g + 32; ++m) u += blk[(size_t)m * ld + t] * xk[m];
    __syncthreads();
    part[g][t] = u;
    __syncthreads();
    if (g == 0) y[(size_t)j * NB + t] -= (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
}

// The same backward substitution as ONE launch (round 3): 79 dependent launches of ~8 us each were 0.6 ms of a cfg-5 iteration.
// Workgroup j owns block row j: it holds Linv_j in registers from the start, takes every x_i (i > j) as it appears, subtracts
// L(i, j)' x_i from its right-hand side (the tile L(i, j) is already in registers by then), then publishes x_j = Linv_j' y_j.
// The hand-off is the DATA itself: x is preset to a sentinel (all-ones bit pattern, a NaN no arithmetic produces), written with
// agent-coherent stores and polled element by element with agent-coherent loads -- one memory round trip per step instead of
// three (store acknowledged, flag stored, flag seen, data loaded), no L2-wide release / acquire.  The sums are grouped exactly as
// in k_trsv_bwd (four partial sums of 32, combined pairwise, block rows in descending order), so the bits are the same.
// Workgroup j waits only for workgroups dispatched BEFORE it (larger j = smaller block index, and dispatch is in order), so the
// launch cannot deadlock whatever share of it is resident; the host still keeps it to nblk <= half the CUs.  An element that
// does not come within 2 s raises *flag = 4 and the host repeats the substitution with the per-step kernels.
#define TRSV_SENTINEL 0xFFFFFFFFFFFFFFFFull
// (y == nullptr: y is row `yrow` of the factor -- the right-hand side went through the factorisation as the system's last row; its
//  sub-diagonal tiles live in Lm, the last diagonal tile in Sm, entries from yrow on are zero: what k_ba_y_from_row extracts)
__global__ __launch_bounds__(512) void k_trsv_bwd_chain(const double *Lm, int ld, int nblk, const double *Linv, const double *y, double *x, int *flag,
                                                        const double *Sm = nullptr, int yrow = 0)
{
    __shared__ double xk[NB], part[4][NB];
    const int t = threadIdx.x & 127, g = threadIdx.x >> 7;
    const int j = nblk - 1 - (int)blockIdx.x;             // the head of the chain is dispatched first
    double li[32], cur[32], nxt[32];
    {
        const double *Lk = Linv + (size_t)j * NB * NB;
#pragma unroll
        for (int m = 0; m < 32; ++m) li[m] = Lk[(size_t)(32 * g + m) * NB + t];
    }
    double yj = 0.0;
    if (g == 0) {
        const int idx = j * NB + t;
        yj = y ? y[idx] : (idx < yrow ? (j < nblk - 1 ? Lm : Sm)[(size_t)yrow * ld + idx] : 0.0);
    }
    auto fetch = [&](int i, double (&dst)[32]) {
        const double *blk = Lm + ((size_t)i * NB) * ld + (size_t)j * NB;      // L[i, j] tile: rows m, column t
#pragma unroll
        for (int m = 0; m < 32; ++m) dst[m] = blk[(size_t)(32 * g + m) * ld + t];
    };
    if (nblk - 1 > j) fetch(nblk - 1, nxt);
    unsigned long long *xb = reinterpret_cast<unsigned long long *>(x);
    for (int i = nblk - 1; i > j; --i) {
#pragma unroll
        for (int m = 0; m < 32; ++m) cur[m] = nxt[m];
        if (i - 1 > j) fetch(i - 1, nxt);
        if (g == 0) {
            unsigned long long v = __hip_atomic_load(xb + (size_t)i * NB + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == TRSV_SENTINEL) {
                const unsigned long long t0 = wall_clock64();
                do {
                    __builtin_amdgcn_s_sleep(2);
                    v = __hip_atomic_load(xb + (size_t)i * NB + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (wall_clock64() - t0 > 200000000ull || __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) { flag_raise(flag, 4); break; }
                } while (v == TRSV_SENTINEL);
            }
            xk[t] = __longlong_as_double((long long)v);
        }
        __syncthreads();
        double u = 0.0;
#pragma unroll
        for (int m = 0; m < 32; ++m) u += cur[m] * xk[32 * g + m];
        part[g][t] = u;
        __syncthreads();
        if (g == 0) yj -= (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    }
    __syncthreads();
    if (g == 0) xk[t] = yj;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 32; ++m) s += li[m] * xk[32 * g + m];      // zeros above the diagonal
    part[g][t] = s;
    __syncthreads();
    if (g == 0) {
        const double xv = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
        __hip_atomic_store(xb + (size_t)j * NB + t, (unsigned long long)__double_as_longlong(xv), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ======================================================== host side (chol.h) ========================================================
// What only the creation of the streams needs.  panel_mode 0: the panel stream under the bulk streams' mask (rounds 2-4); 1: unmasked, highest priority; 2: masked off the chain's eight CUs only
struct CholSetup { bool carve; int reserved = 8, panel_mode = 1; bool poll_set = false; int poll_mode = 0, poll_sleeps = 1; };
#ifdef RCN_DIAG
// Diagnostic build only (tools/librcn_diag.so, -DRCN_DIAG): every switch of the factorisation, read once by rcn_chol_create.  The
// shipping library reads no environment variable.
static void env_int(const char *name, int &v) { if (const char *e = std::getenv(name)) v = std::atoi(e); }
static void env_bool(const char *name, bool &v) { if (const char *e = std::getenv(name)) v = v ? e[0] != '0' : e[0] == '1'; }      // what is on goes off with 0, what is off goes on with 1
static void chol_read_env(CholState &cs, CholSetup &su)
{
    if (getenv("RCN_NO_CU_MASK")) su.carve = false;
    if (const char *rc = getenv("RCN_RESERVED_CUS")) su.reserved = std::max(8, std::min(64, std::atoi(rc) / 8 * 8));
    env_int("RCN_PANEL_MODE", su.panel_mode);
    su.poll_set = std::getenv("RCN_POLL_MODE") || std::getenv("RCN_POLL_SLEEPS");
    env_int("RCN_POLL_MODE", su.poll_mode);
    env_int("RCN_POLL_SLEEPS", su.poll_sleeps);
    env_bool("RCN_CHOL_SAFE", cs.safe);
    env_bool("RCN_TRSV_CHAIN", cs.trsv_chain);
    env_int("RCN_CHOL_BREAK", cs.brk);
    env_int("RCN_CHOL_CHAIN_STREAM", cs.chain_stream_mode);
    env_bool("RCN_CHOL_PG_PRIO", cs.pg_prio);
    env_int("RCN_CHOL_GATE_IN_KERNEL", cs.gate_in_kernel);
    env_bool("RCN_CHOL_HOSTTIME", cs.host_time);
    env_int("RCN_DIAG_STREAM_PRIO", cs.diag_stream_prio);      // 0: normal priority, 2: a CU mask of all CUs
    int group = 2;      // panels per bulk update of the right-looking regime while many tile rows remain, 2 (K = 256) or 1
    env_int("RCN_CHOL_GROUP", group);
    cs.prm.pair = group >= 2 ? 1 : 0;
    env_int("RCN_CHOL_PAIR_MIN", cs.prm.pair_min);
    env_int("RCN_CHOL_TL", cs.prm.tl_g);
    env_int("RCN_CHOL_TL_MIN", cs.prm.tl_min);
    env_int("RCN_CHOL_PGSTREAM", cs.prm.pg_stream);
    env_int("RCN_CHOL_BULK_BEHIND", cs.prm.bulk_behind);
    env_int("RCN_CHOL_CARVE", cs.prm.carve_rows);
    env_int("RCN_CHOL_DIAG_SERVER", cs.prm.diag_server);
    env_int("RCN_CHOL_WINDOW", cs.prm.window);
    env_int("RCN_CHOL_TL_SERIAL", cs.prm.tl_serial);
    env_int("RCN_CHOL_HEAD_SMALL", cs.prm.head_small);
    env_int("RCN_CHOL_FUSE_TAIL", cs.prm.fuse_tail);
    env_int("RCN_CHOL_PIPE_MIN", cs.prm.pipe_min);
}
#endif

int rcn_chol_create(rcn_ctx *ctx)
{
    CholState &cs = ctx->chol;
    // Streams of the dense factorisation (chol_plan.h).  Throughput work -- the bulk trailing updates (aux) and the
    // two-level regime's panel products below the head rows (panel2) -- runs under a CU mask that leaves a few CUs free (mask
    // bits interleave over the XCDs: bit i -> XCD i % 8, so whole rounds of eight keep the XCDs even): the chain's single-workgroup
    // diagonal kernel (132 KB of LDS) never queues behind resident bulk workgroups.  Round 5: the panel stream, which carries the
    // small kernels the chain WAITS for (in-block panels and columns, block rows of a super-block's inverse, the head rows'
    // product and the update of the next super-diagonal block), is NOT masked any more and gets the highest stream priority: with
    // two bulk workgroups per CU holding every vector register of the masked CUs, its kernels could only start where a bulk
    // workgroup retired -- 40-100 us for a 5-us kernel once a bulk tile lives 165 us (K = 512), measured in the device timeline.
    {
        const int ncu = ctx->prop.multiProcessorCount;
        std::vector<uint32_t> mask((ncu + 31) / 32, 0xFFFFFFFFu);
        if (ncu % 32) mask.back() = (1u << (ncu % 32)) - 1u;
        CholSetup su;
        su.carve = ncu >= 64;
#ifdef RCN_DIAG
        chol_read_env(cs, su);
#endif
        std::vector<uint32_t> mask8 = mask;
        if (su.carve) {
            for (int i = 0; i < su.reserved; ++i) mask[(size_t)i / 32] &= ~(1u << (i % 32));
            mask8[0] &= ~0xFFu;
        }
        if (hipExtStreamCreateWithCUMask(&cs.aux, (uint32_t)mask.size(), mask.data()) != hipSuccess) { (void)hipGetLastError(); cs.aux = nullptr; }
        cs.bulk_cu_mask = mask;      // (a second stream under the same mask is made when a plan asks for it: ensure_chol_plan)
        if (su.panel_mode != 1) {
            const std::vector<uint32_t> &pm = su.panel_mode == 2 ? mask8 : mask;
            if (hipExtStreamCreateWithCUMask(&cs.panel, (uint32_t)pm.size(), pm.data()) != hipSuccess) { (void)hipGetLastError(); cs.panel = nullptr; }
        } else {
            int lo = 0, hi = 0;
            if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
            if (hipStreamCreateWithPriority(&cs.panel, hipStreamNonBlocking, hi) != hipSuccess) { (void)hipGetLastError(); cs.panel = nullptr; }
        }
        if (!cs.panel && hipStreamCreateWithFlags(&cs.panel, hipStreamNonBlocking) != hipSuccess) return RCN_ERR_HIP;
#ifdef RCN_DIAG
        if (su.poll_set) (void)rcn_diag_set_poll(su.poll_mode, su.poll_sleeps);
#endif
    }
    if (!cs.aux && hipStreamCreateWithFlags(&cs.aux, hipStreamNonBlocking) != hipSuccess) return RCN_ERR_HIP;
#ifdef RCN_DIAG
    if (cs.chain_stream_mode && cs.chain_stream_mode != 4 && !cs.chain) {
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
        if (cs.chain_stream_mode == 3) {      // a stream with a CU mask of all CUs: a hardware queue of its own?
            const int ncu = ctx->prop.multiProcessorCount;
            std::vector<uint32_t> full((ncu + 31) / 32, 0xFFFFFFFFu);
            if (ncu % 32) full.back() = (1u << (ncu % 32)) - 1u;
            if (hipExtStreamCreateWithCUMask(&cs.chain, (uint32_t)full.size(), full.data()) != hipSuccess) { (void)hipGetLastError(); cs.chain = nullptr; }
        } else
        if (hipStreamCreateWithPriority(&cs.chain, hipStreamNonBlocking, cs.chain_stream_mode == 2 ? 0 : hi) != hipSuccess) { (void)hipGetLastError(); cs.chain = nullptr; }
    }
#endif
    for (auto &e : cs.ev)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return RCN_ERR_HIP;
    return RCN_OK;
}
void rcn_chol_destroy(rcn_ctx *ctx)
{
    CholState &cs = ctx->chol;
    cs.bulk_map.release(); cs.diag_items.release();
    for (auto &e : cs.ev) if (e) (void)hipEventDestroy(e);
    for (hipStream_t s : {cs.aux, cs.panel, cs.panel2, cs.diag, cs.chain})
        if (s) (void)hipStreamDestroy(s);
}
CholWs rcn_chol_ws(const rcn_ctx *ctx, int nblk)
{
    const size_t ldsi = (size_t)NB * std::max(ctx->chol.prm.tl_g, 1);
    return {(size_t)nblk * NB * NB, 2 * ldsi * ldsi};      // (a super-block's inverse: two buffers alternating by super-step)
}
int rcn_chol_prepare(rcn_ctx *ctx)
{
    if (ctx->chol.prepared) return RCN_OK;
    for (const void *k : {(const void *)k_chol_diag, (const void *)k_chol_diag_server})
        RCN_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, NB * DL * 8));
    for (const void *k : {(const void *)k_gemm_nt_pipe<0, 16>, (const void *)k_gemm_nt_pipe<0, 32>, (const void *)k_gemm_nt_pipe<0, 0>, (const void *)k_gemm_nt_pipe<0, 16, 1>,
                          (const void *)k_gemm_nt_pipe<0, 0, 2>, (const void *)k_gemm_nt_pipe_tail})
        RCN_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, GST * GSTAGE_BYTES));
    ctx->chol.prepared = true;
    return RCN_OK;
}

// The factorisation's schedule for nblk blocks (chol_plan.h): built once per shape and parameter set, its tile maps uploaded once.
static int ensure_chol_plan(rcn_ctx *ctx, int nblk)
{
    CholState &cs = ctx->chol;
    chol::Params prm = cs.prm;
    prm.nblk = nblk;
    if (cs.plan_valid && cs.plan.prm_asked == prm) return RCN_OK;
    cs.plan_valid = false;
    cs.plan = chol::make_plan(prm);
    cs.plan.prm_asked = prm;
    RCN_HIP(hipStreamSynchronize(ctx->stream));          // nobody may still read the old maps
    const size_t nm = std::max<size_t>(cs.plan.maps.size(), 1);
    RCN_HIP(cs.bulk_map.reserve(nm * sizeof(unsigned)));
    if (!cs.plan.maps.empty()) RCN_HIP(hipMemcpy(cs.bulk_map.p, cs.plan.maps.data(), cs.plan.maps.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    if (prm.pg_stream && !cs.panel2) {      // a fourth stream for the first super-step's panel product (the shipping plan has none)
        if (cs.bulk_cu_mask.empty() || hipExtStreamCreateWithCUMask(&cs.panel2, (uint32_t)cs.bulk_cu_mask.size(), cs.bulk_cu_mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            RCN_HIP(hipStreamCreateWithFlags(&cs.panel2, hipStreamNonBlocking));
        }
    }
    if (prm.diag_server && !cs.diag) {      // (tools/ only: the product's plans have no resident workgroup)
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
        if (cs.diag_stream_prio == 0) hi = 0;
        if (cs.diag_stream_prio == 2) {      // a stream with a CU mask of all CUs: a hardware queue of its own?
            const int ncu = ctx->prop.multiProcessorCount;
            std::vector<uint32_t> full((ncu + 31) / 32, 0xFFFFFFFFu);
            if (ncu % 32) full.back() = (1u << (ncu % 32)) - 1u;
            RCN_HIP(hipExtStreamCreateWithCUMask(&cs.diag, (uint32_t)full.size(), full.data()));
        } else
        RCN_HIP(hipStreamCreateWithPriority(&cs.diag, hipStreamNonBlocking, hi));
    }
    {   // the resident diagonal workgroup's list: block, whether the factor itself is stored (last block), ticket, waits
        std::vector<DiagItem> items;
        for (const chol::Op &op : cs.plan.ops) {
            if (op.stream != chol::ST_E || op.kind != chol::DIAG) continue;
            DiagItem it;
            memset(&it, 0, sizeof(it));
            it.kb = op.kb; it.store_L = op.kb == nblk - 1; it.ticket = op.ticket; it.tl = op.tl; it.nw = op.nw;
            for (int i = 0; i < op.nw; ++i) { it.ctr[i] = op.w[i].ctr; it.val[i] = op.w[i].val; }
            items.push_back(it);
        }
        RCN_HIP(cs.diag_items.reserve(std::max<size_t>(items.size(), 1) * sizeof(DiagItem)));
        if (!items.empty()) RCN_HIP(hipMemcpy(cs.diag_items.p, items.data(), items.size() * sizeof(DiagItem), hipMemcpyHostToDevice));
    }
    cs.plan_valid = true;
    return RCN_OK;
}
int rcn_chol_plan(rcn_ctx *ctx, int nblk) { return ensure_chol_plan(ctx, nblk); }
hipStream_t rcn_chol_idle_stream(rcn_ctx *ctx) { return ctx->chol.panel; }
bool rcn_chol_bwd_one_launch(const rcn_ctx *ctx, int nblk) { return ctx->chol.trsv_chain && 2 * nblk <= ctx->prop.multiProcessorCount; }
bool rcn_chol_bwd_gave_up(rcn_ctx *ctx) { return std::exchange(ctx->chol.trsv_chain, false); }

extern "C" int rcn_ba_factor_plan(int32_t n_blocks, const int32_t *params, int32_t *ops, int64_t ops_cap, uint32_t *maps, int64_t maps_cap, int64_t *n_ops, int64_t *n_maps)
{
    if (n_blocks < 1 || n_blocks > 16383 || !n_ops || !n_maps) return RCN_ERR_ARG;
    chol::Params prm = params ? chol::params_from_array(params) : chol::Params();
    prm.nblk = n_blocks;
    if (prm.tl_g < 0 || prm.tl_g == 1 || prm.tl_g > 16 || prm.pipe_min < 1) return RCN_ERR_ARG;
    const chol::Plan pl = chol::make_plan(prm);
    *n_ops = (int64_t)pl.ops.size();
    *n_maps = (int64_t)pl.maps.size();
    if ((int64_t)pl.ops.size() > ops_cap || (int64_t)pl.maps.size() > maps_cap || (!ops && !pl.ops.empty()) || (!maps && !pl.maps.empty())) return RCN_ERR_ARG;
    for (size_t i = 0; i < pl.ops.size(); ++i) {
        const chol::Op &o = pl.ops[i];
        int32_t *w = ops + RCN_PLAN_OP_WORDS * i;
        const int32_t v[RCN_PLAN_OP_WORDS] = {o.kind, o.stream, o.ticket, o.kb, o.first, o.m, o.dj, o.nst, o.map_off, o.map_n, o.g, o.pos, o.nw,
                                              o.w[0].ctr, o.w[0].val, o.w[1].ctr, o.w[1].val, o.w[2].ctr, o.w[2].val, o.w[3].ctr, o.w[3].val, o.w[4].ctr, o.w[4].val, o.w[5].ctr, o.w[5].val,
                                              o.tl, o.awaited, o.fuse_with, o.small};
        memcpy(w, v, sizeof(v));
    }
    if (!pl.maps.empty()) memcpy(maps, pl.maps.data(), pl.maps.size() * sizeof(uint32_t));
    return RCN_OK;
}

static bool trsv_in_diag(const rcn_ctx *ctx, const CholSystem &s) { return s.nblk == 1 && s.rhs_row && s.chain && s.fused_finish && ctx->chol.trsv_chain; }      // (one block: the backward substitution rides in the diagonal kernel's launch)

// Dense Cholesky of the padded system: the schedule is DATA (chol_plan.h) -- a list of tile operations in an order that is a
// correct sequential algorithm, each with its stream (A: the chain of diagonal blocks and critical tiles, B: panels and
// columns, C: bulk trailing updates) and the device counters it waits for, derived from the tiles it reads and writes.
// Hand-offs (Gate, above): every stream owns a progress counter; an operation publishes "everything before me on my stream
// is done" with its FIRST thread (stream order has completed that work and the kernel boundary has released its writes) and
// waits for other streams' counters itself -- inside the kernel on the chain and for the small kernels, in a ONE-WAVE gate
// kernel in front of a pipelined launch (a grid of a thousand workgroups that spins while it holds its CU slots could keep
// the very kernel it waits for from becoming resident).  A bulk update counts the tiles the next steps read first out one
// by one (two classes, flag[5], flag[6]).  A wait that times out (2 s: a runtime that does not let the three streams
// progress side by side) raises flag 3; the caller then repeats the factorisation on ONE stream in list order (safe), and runs
// every later one that way (CholState::safe).  Same bits either way: no operation's arithmetic depends on where it runs.
hipError_t rcn_chol_factorise(rcn_ctx *ctx, const CholSystem &s, bool safe)
{
    CholState &cs = ctx->chol;
    hipStream_t st = ctx->stream;
    const int n = s.n, npad = s.npad, nblk = s.nblk;
    const size_t si_elems = rcn_chol_ws(ctx, nblk).si / 2;
    // (the chain on a high-priority stream of the library's own, forked from and joined to the caller's: RCN_CHOL_CHAIN_STREAM, tools/)
    const bool own_chain = !safe && cs.chain_stream_mode && cs.chain;
    hipStream_t str[chol::N_STREAMS] = {own_chain ? cs.chain : st, safe ? st : cs.panel, safe ? st : cs.aux, safe ? st : cs.panel2, safe ? st : cs.diag};
#ifdef RCN_DIAG
    const bool swap_ab = !safe && cs.chain_stream_mode == 4;      // the chain on the panel stream's handle, the panels on the caller's stream
    if (swap_ab) { str[0] = cs.panel; str[1] = st; }
#else
    const bool swap_ab = false;
#endif
    int *const ctr_base = s.flag + 12;          // the streams' progress counters and the two head-tile counters (fused_finish: cleared by the launch that finished S)
    int *ctr[chol::N_CTR];
    for (int c = 0; c < chol::N_CTR; ++c) ctr[c] = ctr_base + c;
    const chol::Plan &plan = cs.plan;
    if (!safe) {
        hipError_t e = hipEventRecord(cs.ev[0], st);
        if ((own_chain || swap_ab) && e == hipSuccess) e = hipStreamWaitEvent(str[0], cs.ev[0], 0);
        for (int s2 = 1; s2 < chol::N_STREAMS && e == hipSuccess; ++s2)
            if (plan.n_ops[s2] && str[s2] != st) e = hipStreamWaitEvent(str[s2], cs.ev[0], 0);     // the other streams start behind everything queued so far
        if (e != hipSuccess) return e;
    }
    const unsigned *maps = cs.bulk_map.as<unsigned>();
    const int ldsi = NB * std::max(plan.prm.tl_g, 1);
    const size_t lds_pipe = GST * GSTAGE_BYTES;
#ifdef RCN_DIAG
    const auto th0 = std::chrono::steady_clock::now();
#endif
    // a bulk update whose launch carries the next super-step's panel product as its tail (chol_plan.h, fuse_with): found per host
    std::vector<int> tail_of(plan.ops.size(), -1);
    if (!safe)
        for (size_t i = 0; i < plan.ops.size(); ++i)
            if (plan.ops[i].fuse_with >= 0) tail_of[(size_t)plan.ops[i].fuse_with] = (int)i;
    auto gate_of = [&](const chol::Op &o2, bool with_pub) {
        Gate g2 = gate_none(s.flag);
        g2.nw = o2.nw;
        for (int i = 0; i < o2.nw; ++i) { g2.c[i] = ctr[o2.w[i].ctr]; g2.n[i] = o2.w[i].val; }
        if (with_pub) { g2.pub = ctr[o2.stream]; g2.pubval = o2.ticket - 1; }
        return g2;
    };
    // the diagonal blocks: ONE resident workgroup for all of them (k_chol_diag_server), started in front of everything else
    const bool server = !safe && plan.n_ops[chol::ST_E] > 0;
    if (server) {
        const int n_active = s.rhs_row ? n + 1 : n;
        k_chol_diag_server<<<1, 64 * CDW, NB * DL * 8, str[chol::ST_E]>>>(s.S, npad, s.Linv, s.flag, cs.diag_items.as<DiagItem>(), plan.n_ops[chol::ST_E], ctr_base, chol::ST_E, n_active);
    }
    for (size_t oi = 0; oi < plan.ops.size(); ++oi) {
        const chol::Op &op = plan.ops[oi];
        if (!safe && op.fuse_with >= 0) continue;      // its tiles went out with the bulk update in front of it
        if (server && op.stream == chol::ST_E) continue;      // the resident workgroup's
        hipStream_t sq = str[op.stream];
        Gate g = safe ? gate_none(s.flag) : gate_of(op, true);
#ifdef RCN_DIAG
        // RCN_CHOL_BREAK=1: the critical tile of step 1 waits for a count that never comes -- the test of the fallback
        if (!safe && cs.brk && op.kind == chol::TRSM_Q && op.stream == chol::ST_A && op.kb == 1 && g.nw > 0) g.n[0] = 1 << 30;
#endif
        // Where the wait stands.  On the chain (stream A) inside the kernel: its grids are small and nothing is saved by a launch in
        // front.  On every other stream in a ONE-WAVE gate kernel in front of the work, never inside it: a grid of hundreds of
        // workgroups that spins while it holds its CU slots -- and polls one counter from every workgroup -- could keep the very
        // kernel it waits for from becoming resident, and slows the chain's kernels beside it (measured: the critical-tile
        // kernels took 11 us instead of 4 with the panel kernels spinning next to them).
        const bool in_kernel = (op.stream == chol::ST_A && cs.gate_in_kernel >= 0) || cs.gate_in_kernel > 0;      // (-1, tools/ only: a gate kernel in front on the chain too)
        const bool pipe_kind = ((op.kind == chol::TRSM_PIPE || op.kind == chol::UPD_PIPE || op.kind == chol::PGEMM) && !op.small) || op.kind == chol::PUBLISH;
        Gate gk = gate_none(s.flag);           // what the kernel itself gets
        if (!safe) {
            if (pipe_kind) {
                if (op.nw > 0 || op.awaited) k_ring_gate<<<1, 64, 0, sq>>>(g);
            } else if (in_kernel) gk = g;
            else {
                if (op.nw > 0) k_ring_gate<<<1, 64, 0, sq>>>(g);
                gk.pub = g.pub; gk.pubval = g.pubval;      // publishing costs one store: no launch for that alone
            }
        }
        const int gq = 32 * ((4 * op.m + 7) / 8);                          // k_gemm_q: strips of 32 rows on the eight XCD slots
        const int prio = (op.stream == chol::ST_C || (op.stream == chol::ST_D && !cs.pg_prio)) ? 0 : PIPE_PRIO;
        switch (op.kind) {
        case chol::DIAG: {
            // (active rows of the block: the system's n rows, and the right-hand-side row behind them when it rides along)
            const int nact = std::min(NB, (s.rhs_row ? n + 1 : n) - op.kb * NB);
            k_chol_diag<<<1, 64 * CDW, NB * DL * 8, sq>>>(s.S, npad, op.kb, s.Linv, s.flag, op.kb == nblk - 1, gk, nact, op.tl,
                                                           trsv_in_diag(ctx, s) ? s.rhs : nullptr, n);
            break;
        }
        case chol::TRSM_Q:
            k_gemm_q<0><<<gq, 256, 0, sq>>>(s.S, s.L, npad, op.kb, op.first, op.m, s.Linv, gk, 1, op.tl);
            break;
        case chol::UPD_Q:
            k_gemm_q<1><<<gq, 256, 0, sq>>>(s.S, s.L, npad, op.kb, op.first, op.m, s.Linv, gk, op.dj, op.tl);
#ifdef RCN_DIAG
            if (cs.brk == 2 && op.stream == chol::ST_A && op.kb == 1 && !safe) k_diag_poison<<<1, 1, 0, sq>>>(s.S, npad, op.kb + 1);      // the next diagonal kernel meets a NaN pivot AFTER the timeout
#endif
            break;
        case chol::TRSM_PIPE:
            k_gemm_nt_pipe<0, 16, 1><<<op.map_n, 256, lds_pipe, sq>>>(s.L, s.S, npad, op.kb, maps + op.map_off, prio, nullptr, s.Linv, NB, 16, op.tl);
            break;
        case chol::UPD_PIPE: {
            if (op.small) { k_gemm_qm<1><<<16 * op.map_n, 256, 0, sq>>>(s.S, s.L, npad, op.kb, maps + op.map_off, op.nst / 16, nullptr, 0, gk, op.tl); break; }
            int *sg = (op.stream == chol::ST_C && !safe) ? ctr[chol::CTR_SIG1] : nullptr;
            // (a launch with a tail first, whatever its K: with two panels per super-step the host is a K = 256 update, and the
            //  compile-time form of that length has no tail -- the product riding in it was skipped above and must not be lost)
            if (tail_of[oi] >= 0) {
                const chol::Op &tp = plan.ops[(size_t)tail_of[oi]];
                k_gemm_nt_pipe_tail<<<op.map_n + tp.map_n, 256, lds_pipe, sq>>>(s.S, s.L, npad, op.kb, op.nst, maps + op.map_off, op.map_n, prio, sg, op.tl,
                                                                                  tp.kb, maps + tp.map_off, s.SI + (size_t)tp.dj * si_elems, ldsi, gate_of(tp, false), tp.tl);
            }
            else if (op.nst == 16) k_gemm_nt_pipe<0, 16><<<op.map_n, 256, lds_pipe, sq>>>(s.S, s.L, npad, op.kb, maps + op.map_off, prio, sg, nullptr, 0, 16, op.tl);
            else if (op.nst == 32) k_gemm_nt_pipe<0, 32><<<op.map_n, 256, lds_pipe, sq>>>(s.S, s.L, npad, op.kb, maps + op.map_off, prio, sg, nullptr, 0, 32, op.tl);
            else k_gemm_nt_pipe<0, 0><<<op.map_n, 256, lds_pipe, sq>>>(s.S, s.L, npad, op.kb, maps + op.map_off, prio, sg, nullptr, 0, op.nst, op.tl);
            break;
        }
        case chol::SINV:
            k_sinv<<<8 * op.pos + 1, 512, 0, sq>>>(s.L, npad, s.Linv, s.SI + (size_t)op.dj * si_elems, ldsi, op.kb, op.pos, gk, op.tl);
            break;
        case chol::PGEMM:
            if (op.small) { k_gemm_qm<2><<<16 * op.map_n, 256, 0, sq>>>(s.S, s.L, npad, op.kb, maps + op.map_off, 0, s.SI + (size_t)op.dj * si_elems, ldsi, gk, op.tl); break; }
            k_gemm_nt_pipe<0, 0, 2><<<op.map_n, 256, lds_pipe, sq>>>(s.L, s.S, npad, op.kb, maps + op.map_off, prio, nullptr, s.SI + (size_t)op.dj * si_elems, ldsi, 0, op.tl);
            break;
        case chol::PUBLISH:
            break;
        }
    }
#ifdef RCN_DIAG
    if (cs.host_time) fprintf(stderr, "factorise: %zu operations enqueued in %.3f ms of host time\n", plan.ops.size(), std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count());
#endif
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || safe) return e;
    // the chain continues (triangular solves) behind the last kernels of the other streams
    for (int s2 = 1; s2 < chol::N_STREAMS && e == hipSuccess; ++s2) {
        if (!plan.n_ops[s2]) continue;
        if (str[s2] == st) continue;
        e = hipEventRecord(cs.ev[s2], str[s2]);
        if (e == hipSuccess) e = hipStreamWaitEvent(str[0], cs.ev[s2], 0);
    }
    if ((own_chain || swap_ab) && e == hipSuccess) {
        e = hipEventRecord(cs.ev[5], str[0]);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, cs.ev[5], 0);
    }
    return e;
}

// The triangular solves behind the factorisation, on ctx->stream; the solution is left in s.rhs.
// (rhs_row + chain, the default: the sentinel was left by the launch that finished S and the chain kernel reads y out of the factor's
//  last row itself -- no launch in between; otherwise the caller has taken y out of that row, or the forward substitution runs here)
hipError_t rcn_chol_substitute(rcn_ctx *ctx, const CholSystem &s)
{
    hipStream_t st = ctx->stream;
    const int n = s.n, npad = s.npad, nblk = s.nblk;
    const bool y_in_row = s.chain && s.fused_finish;
    if (!s.rhs_row) for (int kb = 0; kb < nblk; ++kb) k_trsv_fwd<<<nblk - kb, 128, 0, st>>>(s.L, npad, kb, s.Linv, s.rhs, s.yc);
    if (s.chain) {
        if (!s.rhs_row)      // the sentinel
            if (hipError_t e = hipMemsetAsync(s.rhs, 0xFF, sizeof(double) * npad, st)) return e;
        if (trsv_in_diag(ctx, s)) {}      // done by k_chol_diag
        else if (y_in_row) k_trsv_bwd_chain<<<nblk, 512, 0, st>>>(s.L, npad, nblk, s.Linv, nullptr, s.rhs, s.flag, s.S, n);
        else k_trsv_bwd_chain<<<nblk, 512, 0, st>>>(s.L, npad, nblk, s.Linv, s.yc, s.rhs, s.flag);
    }
    else for (int kb = nblk - 1; kb >= 0; --kb) k_trsv_bwd<<<kb + 1, 512, 0, st>>>(s.L, npad, kb, s.Linv, s.yc, s.rhs);
    return hipGetLastError();
}
