// tools/chol_solve_check.hip -- S x = b through chol.h alone, for tests/test_chol_solve_gpu.py: a DRIVER, not a judge.  It owns an rcn_ctx,
// sets the schedule's parameters per case, presents the system in one of the three ways ba.hip does, runs rcn_chol_factorise and
// rcn_chol_substitute on ctx->stream and writes what came out; every numerical verdict is the test's (tests/chol_ref.py).
//
//   chol_solve_check DIR
//
// DIR/cases.txt, one case per line (lines that start with # are skipped):
//   name system n mode safe trsv_chain dump tl_g tl_min pair pair_min pipe_min head_small fuse_tail
// DIR/<system>.S (n x n float64, row-major, little-endian) and DIR/<system>.b (n float64): several cases may name one system.
//   mode  plain  rhs_row = false: identity on the padded diagonal, rhs = b padded with zeros, forward substitution in rcn_chol_substitute
//                (the only mode when n is a multiple of 128)
//         row    rhs_row = true, fused_finish = false: row n of S is [b, RCN_RHS_BETA]; y is taken out of row n of the factor into yc
//                behind the factorisation (what ba.hip's k_ba_y_from_row does), with the one-launch substitution's sentinel in rhs
//         fused  rhs_row and fused_finish = true, the shipping default: flag words, padding rows, row n and the sentinel are left the way
//                the Schur finish launch leaves them, rcn_chol_substitute reads y itself (one block: inside k_chol_diag)
//   safe  1: the factorisation on ctx->stream alone, in list order.  As in ba.hip, plans of up to two blocks run that way regardless.
//   dump  1: also DIR/<name>.L, .Sf (npad x npad each) and .Linv (nblk tiles of 128 x 128)
// Writes DIR/<name>.x (n float64) and DIR/<name>.out: "flag nblk schedule wall_ms" -- flag[0] as the device left it, schedule 0 = as
// asked, 1 = repeated on one stream because a hand-off timed out (flag 3: what ba.hip does), wall_ms = host time around factorise +
// substitute + synchronise.  L and the upper triangle of S start as NaN: the unit's contract is the lower triangle, and nothing it reads
// may be something it has not been given or has not written.
// Exit code: 0 when every case ran, 1 on the first HIP error, 2 on a case list it cannot read.  No numerical decision is made here.
#include "../reconstructor_amd/csrc/chol.hip"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#define CK(call)                                                                                              \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s (case %s)\n", #call, hipGetErrorString(e_), g_case.c_str()); return 1; } \
    } while (0)
static std::string g_case = "-";

// y out of row n of the factor (sub-diagonal tiles live in L, the last diagonal tile in S) and, on request, the sentinel of the
// one-launch backward substitution: ba.hip's k_ba_y_from_row
__global__ void k_y_from_row(const double *S, const double *L, double *yc, double *rhs, int n, int npad, int sentinel)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= npad) return;
    const int last0 = (npad / NB - 1) * NB;
    yc[j] = j < n ? (j < last0 ? L : S)[(size_t)n * npad + j] : 0.0;
    if (sentinel) reinterpret_cast<unsigned long long *>(rhs)[j] = TRSV_SENTINEL;
}

static bool read_doubles(const std::string &path, std::vector<double> &v, size_t count)
{
    v.resize(count);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = fread(v.data(), sizeof(double), count, f);
    const bool end = fgetc(f) == EOF;
    fclose(f);
    return got == count && end;
}
static bool write_doubles(const std::string &path, const double *p, size_t count)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = fwrite(p, sizeof(double), count, f);
    return fclose(f) == 0 && put == count;
}

struct Case { std::string name, system, mode; int n, safe, trsv_chain, dump, tl_g, tl_min, pair, pair_min, pipe_min, head_small, fuse_tail; };

static int run(const std::string &dir)
{
    std::vector<Case> cases;
    {
        std::ifstream in(dir + "/cases.txt");
        if (!in) { fprintf(stderr, "cannot read %s/cases.txt\n", dir.c_str()); return 2; }
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream ls(line);
            Case c;
            if (!(ls >> c.name >> c.system >> c.n >> c.mode >> c.safe >> c.trsv_chain >> c.dump >> c.tl_g >> c.tl_min >> c.pair >> c.pair_min >> c.pipe_min >> c.head_small >> c.fuse_tail)) {
                fprintf(stderr, "cases.txt: cannot parse \"%s\"\n", line.c_str());
                return 2;
            }
            const bool mode_ok = c.mode == "plain" || c.mode == "row" || c.mode == "fused";
            // (the limits of rcn_ba_factor_plan; a row mode needs a padding row for the right-hand side)
            if (!mode_ok || c.n < 1 || c.n > 16383 * NB || c.tl_g < 0 || c.tl_g == 1 || c.tl_g > 16 || c.pipe_min < 1 || (c.mode != "plain" && c.n % NB == 0)) {
                fprintf(stderr, "cases.txt: case %s cannot be run as asked\n", c.name.c_str());
                return 2;
            }
            cases.push_back(c);
        }
    }
    rcn_ctx ctx_obj;
    rcn_ctx *ctx = &ctx_obj;
    ctx->device = 0;
    CK(hipSetDevice(ctx->device));
    CK(hipGetDeviceProperties(&ctx->prop, ctx->device));
    if (std::string(ctx->prop.gcnArchName).rfind("gfx950", 0) != 0) { fprintf(stderr, "not a gfx950 device: %s\n", ctx->prop.gcnArchName); return 1; }
    CK(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    hipStream_t st = ctx->stream;
    if (rcn_chol_create(ctx) != RCN_OK) { fprintf(stderr, "rcn_chol_create failed\n"); return 1; }
    if (rcn_chol_prepare(ctx) != RCN_OK) { fprintf(stderr, "rcn_chol_prepare: %s\n", ctx->err.c_str()); return 1; }
    const chol::Params shipped = ctx->chol.prm;
    {   // the code object is loaded by the first launch: not inside a case's wall time
        double *w;
        CK(hipMalloc(&w, 4 * NB * sizeof(double)));
        k_y_from_row<<<1, NB, 0, st>>>(w, w, w + NB, w + 2 * NB, 0, NB, 1);
        CK(hipStreamSynchronize(st));
        CK(hipFree(w));
    }
    const double qnan = std::nan("");
    std::string have_system;
    std::vector<double> hS, hb;
    for (const Case &c : cases) {
        g_case = c.name;
        const int n = c.n, npad = std::max(NB, (n + NB - 1) / NB * NB), nblk = npad / NB;
        const size_t N = (size_t)npad * npad;
        if (have_system != c.system + "/" + std::to_string(n)) {
            if (!read_doubles(dir + "/" + c.system + ".S", hS, (size_t)n * n) || !read_doubles(dir + "/" + c.system + ".b", hb, (size_t)n)) {
                fprintf(stderr, "case %s: cannot read system %s of size %d\n", c.name.c_str(), c.system.c_str(), n);
                return 2;
            }
            have_system = c.system + "/" + std::to_string(n);
        }
        // ---- the context's own switches, set directly
        CholState &cs = ctx->chol;
        cs.prm = shipped;
        cs.prm.tl_g = c.tl_g; cs.prm.tl_min = c.tl_min; cs.prm.pair = c.pair; cs.prm.pair_min = c.pair_min; cs.prm.pipe_min = c.pipe_min;
        cs.prm.head_small = c.head_small; cs.prm.fuse_tail = c.fuse_tail;
        cs.trsv_chain = c.trsv_chain != 0;
        if (rcn_chol_plan(ctx, nblk) != RCN_OK) { fprintf(stderr, "rcn_chol_plan: %s (case %s)\n", ctx->err.c_str(), c.name.c_str()); return 1; }
        const bool rhs_row = c.mode != "plain", fused = c.mode == "fused";
        const bool chain = rcn_chol_bwd_one_launch(ctx, nblk);
        // ---- the padded system on the host
        std::vector<double> P(N, 0.0), prhs((size_t)npad, 0.0);
        for (int i = 0; i < npad; ++i) {
            double *row = P.data() + (size_t)i * npad;
            if (i < n) memcpy(row, hS.data() + (size_t)i * n, sizeof(double) * (size_t)(i + 1));
            else if (i == n && rhs_row) { memcpy(row, hb.data(), sizeof(double) * (size_t)n); row[n] = RCN_RHS_BETA; }
            else row[i] = 1.0;
            for (int j = i + 1; j < npad; ++j) row[j] = qnan;
        }
        // (fused + one-launch substitution: the finish launch leaves the sentinel where the solution will stand; every other form starts from b)
        const bool sentinel_up_front = fused && chain;
        if (sentinel_up_front) memset(prhs.data(), 0xFF, sizeof(double) * (size_t)n);
        else memcpy(prhs.data(), hb.data(), sizeof(double) * (size_t)n);
        const CholWs ws = rcn_chol_ws(ctx, nblk);
        double *dS, *dL, *dLinv, *dSI, *drhs, *dyc;
        int *dflag;
        CK(hipMalloc(&dS, N * 8)); CK(hipMalloc(&dL, N * 8)); CK(hipMalloc(&dLinv, ws.linv * 8)); CK(hipMalloc(&dSI, ws.si * 8));
        CK(hipMalloc(&drhs, (size_t)npad * 8)); CK(hipMalloc(&dyc, (size_t)npad * 8)); CK(hipMalloc(&dflag, 64 * sizeof(int)));
        const CholSystem sys = {dS, dL, dLinv, dSI, dflag, drhs, dyc, n, npad, nblk, rhs_row, chain, fused};
        bool safe = c.safe != 0;
        int schedule = 0, flag0 = 0;
        double wall_ms = 0.0;
        for (;;) {
            CK(hipMemcpy(dS, P.data(), N * 8, hipMemcpyHostToDevice));
            CK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(dL), 0x7FF80000, 2 * N));      // (a NaN in every entry, and not the substitution's all-ones sentinel)
            CK(hipMemcpy(drhs, prhs.data(), (size_t)npad * 8, hipMemcpyHostToDevice));
            CK(hipMemset(dLinv, 0, ws.linv * 8)); CK(hipMemset(dSI, 0, ws.si * 8));
            CK(hipMemset(dyc, 0, (size_t)npad * 8)); CK(hipMemset(dflag, 0, 64 * sizeof(int)));
            CK(hipDeviceSynchronize());
            const auto t0 = std::chrono::steady_clock::now();
            CK(rcn_chol_factorise(ctx, sys, safe || nblk <= 2));
            if (rhs_row && !(chain && fused)) k_y_from_row<<<(npad + 255) / 256, 256, 0, st>>>(dS, dL, dyc, drhs, n, npad, chain ? 1 : 0);
            CK(rcn_chol_substitute(ctx, sys));
            CK(hipStreamSynchronize(st));
            wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            CK(hipGetLastError());
            CK(hipMemcpy(&flag0, dflag, sizeof(int), hipMemcpyDeviceToHost));
            if (flag0 != 3 || safe) break;
            safe = true;        // a hand-off between the streams timed out: once more on one stream, as ba.hip does
            schedule = 1;
        }
        std::vector<double> x((size_t)npad);
        CK(hipMemcpy(x.data(), drhs, (size_t)npad * 8, hipMemcpyDeviceToHost));
        bool wrote = write_doubles(dir + "/" + c.name + ".x", x.data(), (size_t)n);
        if (c.dump) {
            std::vector<double> buf(N);
            CK(hipMemcpy(buf.data(), dL, N * 8, hipMemcpyDeviceToHost));
            wrote &= write_doubles(dir + "/" + c.name + ".L", buf.data(), N);
            CK(hipMemcpy(buf.data(), dS, N * 8, hipMemcpyDeviceToHost));
            wrote &= write_doubles(dir + "/" + c.name + ".Sf", buf.data(), N);
            buf.resize(ws.linv);
            CK(hipMemcpy(buf.data(), dLinv, ws.linv * 8, hipMemcpyDeviceToHost));
            wrote &= write_doubles(dir + "/" + c.name + ".Linv", buf.data(), ws.linv);
        }
        {
            FILE *f = fopen((dir + "/" + c.name + ".out").c_str(), "w");
            wrote &= f && fprintf(f, "%d %d %d %.6f\n", flag0, nblk, schedule, wall_ms) > 0;
            if (f) wrote &= fclose(f) == 0;
        }
        if (!wrote) { fprintf(stderr, "case %s: cannot write the results\n", c.name.c_str()); return 2; }
        printf("%-28s n %5d nblk %3d %-5s %s%s flag %d schedule %d  %.3f ms\n", c.name.c_str(), n, nblk, c.mode.c_str(), (safe || nblk <= 2) ? "one stream" : "three streams",
               chain ? ", one-launch substitution" : ", per-step substitution", flag0, schedule, wall_ms);
        fflush(stdout);
        CK(hipFree(dS)); CK(hipFree(dL)); CK(hipFree(dLinv)); CK(hipFree(dSI)); CK(hipFree(drhs)); CK(hipFree(dyc)); CK(hipFree(dflag));
    }
    g_case = "-";
    CK(hipStreamSynchronize(st));
    rcn_chol_destroy(ctx);
    CK(hipStreamDestroy(ctx->own_stream));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: chol_solve_check DIR\n"); return 2; }
    return run(argv[1]);
}
