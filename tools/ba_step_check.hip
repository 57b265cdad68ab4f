// tools/ba_step_check.hip -- one Levenberg-Marquardt iteration of rcn_int_ba_solve copied out, for tests/test_ba_step_gpu.py: a DRIVER,
// not a judge.  It owns an rcn_ctx, sets the options and the probe (BaProbe, rcn_internal.h) per case, calls the product's own
// rcn_int_ba_solve -- csrc/ba.hip and csrc/chol.hip as the library compiles them, included below, no RCN_DIAG -- and writes what the
// probe brought back; every numerical verdict is the test's (tests/ba_ref.py).  No kernel and no launch decision is repeated here.
//
//   ba_step_check DIR
//
// DIR/cases.txt, one case per line (lines that start with # are skipped):
//   name scene iteration intrinsics_mode fix_cam0_pose fix_cam1_translation jacobi_scaling focal_upper_bound initial_radius [min_lm_diagonal max_lm_diagonal [loss_kind loss_scale]]
// (the optional columns come in pairs: without the first pair both diagonals stay as rcn_ba_default_options gives them, like every other
//  option; max_iterations at least `iteration`.  The second pair, which needs the first in front of it, is the robust loss of the solve,
//  rcn_ba_loss's kind and scale: absent, there is none.  With it the case also writes DIR/<name>.weights, rho'(s) per observation at the
//  point where the solve ended, and four "loss_*" lines of the report into the .meta).
// DIR/<scene>.dims ("n_cams n_points n_obs" as text), .poses .intr .pts .uv (float64, little-endian) and .ocam .opt (int32): several
// cases may name one scene -- the pair lists of the second are then the reused ones, as in the product.
// Writes DIR/<name>.meta ("key value" lines: what the probe recorded as integers, the summary's iteration count and termination) and
// one raw file per captured array, DIR/<name>.<array>: float64, except int32 for flag, flag_b, cam_off, cam_dim, cols, pk_off, uint32 for
// tickets, tickets_b and uint64 for pk_list.
// Exit code: 0 when every case ran, 1 on the first HIP error or a solve that returned an error, 2 on a case it cannot read or write.
#include "../reconstructor_amd/csrc/chol.hip"
#include "../reconstructor_amd/csrc/ba.hip"
#include "../reconstructor_amd/csrc/ba_tied.hip"
#include <fstream>
#include <sstream>

#define CKT(call)                                                                                             \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "%s: %s (case %s)\n", #call, hipGetErrorString(e_), g_case.c_str()); return 1; } \
    } while (0)
static std::string g_case = "-";

template <class T> static bool read_raw(const std::string &path, std::vector<T> &v, size_t count)
{
    v.resize(count);
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    const size_t got = count ? fread(v.data(), sizeof(T), count, f) : 0;
    const bool end = fgetc(f) == EOF;
    fclose(f);
    return got == count && end;
}
template <class T> static bool write_raw(const std::string &path, const std::vector<T> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = v.empty() ? 0 : fwrite(v.data(), sizeof(T), v.size(), f);
    return fclose(f) == 0 && put == v.size();
}

struct StepCase { std::string name, scene; int iteration, mode, fix0, fix1, jacobi; double ub, radius, lm_lo, lm_hi; bool lm_given; int loss_kind; double loss_scale; bool loss_given; };
struct StepScene { std::string name; int nc = 0, np = 0, no = 0; std::vector<double> poses, intr, pts, uv; std::vector<int> ocam, opt; };

static int run(const std::string &dir)
{
    std::vector<StepCase> cases;
    {
        std::ifstream in(dir + "/cases.txt");
        if (!in) { fprintf(stderr, "cannot read %s/cases.txt\n", dir.c_str()); return 2; }
        std::string line;
        while (std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            std::istringstream ls(line);
            StepCase c;
            if (!(ls >> c.name >> c.scene >> c.iteration >> c.mode >> c.fix0 >> c.fix1 >> c.jacobi >> c.ub >> c.radius) || c.iteration < 1 || c.iteration > 150 ||
                (c.mode != 0 && c.mode != 1)) {
                fprintf(stderr, "cases.txt: cannot parse \"%s\"\n", line.c_str());
                return 2;
            }
            // (optional trailing columns: both or neither, and nothing behind them)
            c.lm_given = false;
            c.loss_given = false; c.loss_kind = 0; c.loss_scale = 0.0;
            std::string rest;
            if (ls >> rest) {
                std::istringstream lo(rest);
                if (!(lo >> c.lm_lo) || !lo.eof() || !(ls >> c.lm_hi) || !(c.lm_lo >= 0.0) || !(c.lm_hi >= c.lm_lo)) {
                    fprintf(stderr, "cases.txt: cannot parse \"%s\"\n", line.c_str());
                    return 2;
                }
                c.lm_given = true;
                if (ls >> rest) {
                    std::istringstream lk(rest);
                    if (!(lk >> c.loss_kind) || !lk.eof() || !(ls >> c.loss_scale) || (ls >> rest)) {
                        fprintf(stderr, "cases.txt: cannot parse \"%s\"\n", line.c_str());
                        return 2;
                    }
                    c.loss_given = true;
                }
            }
            cases.push_back(c);
        }
    }
    rcn_ctx ctx_obj;
    rcn_ctx *ctx = &ctx_obj;
    ctx->device = 0;
    CKT(hipSetDevice(ctx->device));
    CKT(hipGetDeviceProperties(&ctx->prop, ctx->device));
    if (std::string(ctx->prop.gcnArchName).rfind("gfx950", 0) != 0) { fprintf(stderr, "not a gfx950 device: %s\n", ctx->prop.gcnArchName); return 1; }
    // (what rcn_create does for the BA: ctx.hip)
    CKT(hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking));
    ctx->stream = ctx->own_stream;
    if (rcn_chol_create(ctx) != RCN_OK) { fprintf(stderr, "rcn_chol_create failed\n"); return 1; }
    CKT(hipEventCreateWithFlags(&ctx->ba_pair_ev, hipEventDisableTiming));
    for (auto &e : ctx->ba_tev) CKT(hipEventCreate(&e));
    ctx->ba_ev_made = true;
    CKT(hipHostMalloc(reinterpret_cast<void **>(&ctx->ba_host_scal), 16 * sizeof(double), hipHostMallocDefault));
    memset(ctx->ba_host_scal, 0, 16 * sizeof(double));

    StepScene sc;
    for (const StepCase &c : cases) {
        g_case = c.name;
        if (sc.name != c.scene) {
            std::ifstream dims(dir + "/" + c.scene + ".dims");
            if (!(dims >> sc.nc >> sc.np >> sc.no) || sc.nc < 1 || sc.np < 0 || sc.no < 0) { fprintf(stderr, "case %s: cannot read %s.dims\n", c.name.c_str(), c.scene.c_str()); return 2; }
            const std::string b = dir + "/" + c.scene;
            if (!read_raw(b + ".poses", sc.poses, 6 * (size_t)sc.nc) || !read_raw(b + ".intr", sc.intr, 6 * (size_t)sc.nc) || !read_raw(b + ".pts", sc.pts, 3 * (size_t)sc.np) ||
                !read_raw(b + ".uv", sc.uv, 2 * (size_t)sc.no) || !read_raw(b + ".ocam", sc.ocam, (size_t)sc.no) || !read_raw(b + ".opt", sc.opt, (size_t)sc.no)) {
                fprintf(stderr, "case %s: cannot read scene %s\n", c.name.c_str(), c.scene.c_str());
                return 2;
            }
            sc.name = c.scene;
        }
        // the solve updates its parameter arrays in place: every case starts from the scene's
        std::vector<double> poses = sc.poses, intr = sc.intr, pts = sc.pts;
        rcn_ba_problem pb;
        memset(&pb, 0, sizeof(pb));
        pb.n_cams = sc.nc; pb.n_points = sc.np; pb.n_obs = sc.no;
        pb.poses = poses.data(); pb.intrinsics = intr.data(); pb.points = pts.data();
        pb.obs_uv = sc.uv.data(); pb.obs_cam = sc.ocam.data(); pb.obs_pt = sc.opt.data();
        rcn_ba_options o;
        rcn_ba_default_options(sc.nc, &o);
        o.intrinsics_mode = c.mode; o.fix_cam0_pose = c.fix0; o.fix_cam1_translation = c.fix1; o.jacobi_scaling = c.jacobi;
        o.focal_upper_bound = c.ub; o.initial_trust_region_radius = c.radius;
        if (c.lm_given) { o.min_lm_diagonal = c.lm_lo; o.max_lm_diagonal = c.lm_hi; }
        o.max_iterations = std::max(o.max_iterations, c.iteration);
        BaProbe probe;
        probe.iteration = c.iteration;
        ctx->ba_probe = &probe;
        rcn_ba_summary sum;
        const rcn_ba_loss loss{c.loss_kind, 0, c.loss_scale};
        rcn_ba_loss_report rep;
        std::vector<double> weights(c.loss_given ? (size_t)sc.no : 0);
        const int rc = c.loss_given ? rcn_int_ba_solve(ctx, &pb, &o, &sum, nullptr, &loss, &rep, weights.data())
                                    : rcn_int_ba_solve(ctx, &pb, &o, &sum, nullptr);
        ctx->ba_probe = nullptr;
        if (rc != RCN_OK) { fprintf(stderr, "case %s: rcn_int_ba_solve returned %d: %s\n", c.name.c_str(), rc, ctx->err.c_str()); return 1; }
        CKT(hipGetLastError());
        const std::string b = dir + "/" + c.name;
        bool ok = true;
        {
            FILE *f = fopen((b + ".meta").c_str(), "w");
            ok = f != nullptr;
            if (f) {
                const BaProbe &q = probe;
                fprintf(f, "got_a %d\ngot_b %d\nn %d\nnpad %d\ncsplit %d\noffdiag_kernel %d\ndiag_smb %d\nfin %d\nrhs_row %d\nfused_finish %d\nchain %d\npair_path %d\n",
                        q.got_a, q.got_b, q.n, q.npad, q.csplit, q.offdiag_kernel, q.diag_smb, q.fin, q.rhs_row, q.fused_finish, q.chain, q.pair_path);
                fprintf(f, "iterations %d\ntermination %d\npair_lists_reused %d\nbound_projections %d\nradius %.17g\n", sum.iterations, sum.termination, sum.pair_lists_reused,
                        sum.bound_projections, q.radius);
                if (c.loss_given) fprintf(f, "loss_n_obs %lld\nloss_n_beyond_scale %lld\nloss_plain_rms_px %.17g\nloss_max_residual_px %.17g\n", (long long)rep.n_obs,
                                          (long long)rep.n_beyond_scale, rep.plain_rms_px, rep.max_residual_px);
                ok = fclose(f) == 0;
            }
        }
        if (c.loss_given) ok = ok && write_raw(b + ".weights", weights);
        const BaProbe &q = probe;
#define PUT(field) ok = ok && write_raw(b + "." #field, q.field)
        PUT(J); PUT(crot); PUT(Uraw); PUT(gcraw); PUT(Vraw); PUT(gpraw); PUT(sc); PUT(sp); PUT(dgc); PUT(dgp); PUT(Vinv); PUT(gps); PUT(WY); PUT(S); PUT(rhs);
        PUT(flag); PUT(cam_off); PUT(cam_dim); PUT(cols); PUT(pk_off); PUT(tickets); PUT(pk_list);
        PUT(x); PUT(tobs); PUT(stc); PUT(stp); PUT(dlc); PUT(dlp); PUT(poses2); PUT(intr2); PUT(pts2); PUT(crot2); PUT(scal); PUT(flag_b); PUT(tickets_b);
        PUT(trials); PUT(log);
#undef PUT
        if (!ok) { fprintf(stderr, "case %s: cannot write the captures\n", c.name.c_str()); return 2; }
        printf("%-28s %-20s cams %4d points %6d obs %6d n %5d iteration %d: A %d B %d, csplit %d, off-diagonal kernel %d, diagonal SMB %d, fin %d, lists %d\n", c.name.c_str(), c.scene.c_str(),
               sc.nc, sc.np, sc.no, q.n, c.iteration, q.got_a, q.got_b, q.csplit, q.offdiag_kernel, q.diag_smb, q.fin, q.pair_path);
        fflush(stdout);
    }
    g_case = "-";
    CKT(hipStreamSynchronize(ctx->stream));
    for (DevBuf &w : ctx->ba_ws) w.release();
    ctx->ba_loss_ws.release();
    (void)hipEventDestroy(ctx->ba_pair_ev);
    for (auto &e : ctx->ba_tev) (void)hipEventDestroy(e);
    rcn_chol_destroy(ctx);
    (void)hipHostFree(ctx->ba_host_scal);
    CKT(hipStreamDestroy(ctx->own_stream));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: ba_step_check DIR\n"); return 2; }
    return run(argv[1]);
}
