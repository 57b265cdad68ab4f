// ctx.hip -- context lifetime of the C ABI (include/rcn.h).
#include "rcn_internal.h"

#include <cstdlib>

extern "C" {

const char *rcn_version(void)
{
#ifdef RCN_DIAG
    return "reconstructor_amd 0.19 (gfx950) DIAGNOSTIC BUILD";
#else
    return "reconstructor_amd 0.19 (gfx950)";
#endif
}

int rcn_create(int device_id, rcn_ctx **out)
{
    if (!out) return RCN_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n)
        return RCN_ERR_NO_DEVICE;
    rcn_ctx *ctx = new rcn_ctx();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess ||
        hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess) {
        delete ctx;
        return RCN_ERR_NO_DEVICE;
    }
    // the code object holds gfx950 ISA only: fail loudly on anything else
    if (std::string(ctx->prop.gcnArchName).rfind("gfx950", 0) != 0) {
        delete ctx;
        return RCN_ERR_NO_DEVICE;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return RCN_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    if (int rcc = rcn_chol_create(ctx)) { delete ctx; return rcc; }      // the streams and events of the dense factorisation (chol.hip)
    if (hipEventCreateWithFlags(&ctx->ba_pair_ev, hipEventDisableTiming) != hipSuccess) { delete ctx; return RCN_ERR_HIP; }
    for (auto &e : ctx->ba_tev)
        if (hipEventCreate(&e) != hipSuccess) { delete ctx; return RCN_ERR_HIP; }
    ctx->ba_ev_made = true;
    if (hipHostMalloc(reinterpret_cast<void **>(&ctx->ba_host_scal), 16 * sizeof(double), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->ba_host_scal = nullptr; }
    else memset(ctx->ba_host_scal, 0, 16 * sizeof(double));
#ifdef RCN_DIAG
    // Diagnostic build only (tools/librcn_diag.so, -DRCN_DIAG): ablations and alternative device paths.
    // The shipping library reads no environment variable.
    const char *w4 = std::getenv("RCN_COARSE_W4");
    ctx->coarse_w4 = w4 && w4[0] == '1';
    const char *s16 = std::getenv("RCN_COARSE_S16");
    ctx->coarse_shape = s16 ? (s16[0] == '1' ? 1 : 0) : -1;
    const char *i8 = std::getenv("RCN_COARSE_I8");
    ctx->coarse_i8_off = i8 && i8[0] == '0';
    const char *i8s = std::getenv("RCN_COARSE_I8_S16");
    ctx->coarse_i8_shape = i8s ? (i8s[0] == '1' ? 1 : 0) : -1;
    const char *fe = std::getenv("RCN_FORCE_EXACT");
    ctx->force_exact = fe && fe[0] == '1';
    const char *mi8 = std::getenv("RCN_MID_I8");
    ctx->mid_i8_off = mi8 && mi8[0] == '0';
    const char *mi8m = std::getenv("RCN_MID_I8_MFMA");
    ctx->mid_i8_dot4 = mi8m && mi8m[0] == '0';
    const char *rrp = std::getenv("RCN_RERANK_PASS");
    ctx->rerank_pass = rrp && rrp[0] == '1';
    const char *flp = std::getenv("RCN_FILTER_PASS");
    ctx->filter_pass = flp && flp[0] == '1';
    const char *nio = getenv("RCN_MATCH_NO_ORDER");
    ctx->no_item_order = nio && nio[0] == '1';
    const char *ab = std::getenv("RCN_COARSE_ABL");
    ctx->ablate = ab ? std::atoi(ab) : 0;
    const char *bat = std::getenv("RCN_BA_SCHUR_ATOMICS");
    ctx->ba_atomics = bat && bat[0] == '1';
    const char *bps = getenv("RCN_PAIR_SMALL");
    if (bps) ctx->ba_pair_small = bps[0] != '0';
    const char *btf = getenv("RCN_BA_TRSV_FWD");
    ctx->ba_trsv_fwd = btf && btf[0] == '1';
    if (const char *bm = std::getenv("RCN_BA_MIRROR")) if (bm[0] == '0' && ctx->ba_host_scal) { (void)hipHostFree(ctx->ba_host_scal); ctx->ba_host_scal = nullptr; }      // the scalars by copy + synchronisation, as before round 5
    const char *ch = std::getenv("RCN_CHUNK_ROWS");
    if (ch && std::atoll(ch) > 0) ctx->chunk_rows = std::atoll(ch);
    const char *mr = std::getenv("RCN_MID_ROWS");
    if (mr && std::atoll(mr) >= 0) ctx->mid_rows = std::max<long long>(1, std::atoll(mr));
#endif
    memset(&ctx->last_stats, 0, sizeof(ctx->last_stats));
    *out = ctx;
    return RCN_OK;
}

void rcn_destroy(rcn_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    rcn_match_release(ctx);
    rcn_int_ham_release(ctx);
    rcn_int_guided_release(ctx);
    rcn_int_tracks_release(ctx);
    rcn_int_mvs_release(ctx);
    DevBuf *bufs[] = {&ctx->img_table, &ctx->pairs_dev, &ctx->groups_dev, &ctx->cand, &ctx->owner,
                      &ctx->fb_list, &ctx->sv_list, &ctx->counters, &ctx->out_tmp, &ctx->cnt_tmp, &ctx->scale_dev, &ctx->desc_bad, &ctx->kp_ws, &ctx->sg_ws, &ctx->sg_scores, &ctx->gnn_ws, &ctx->gnn_mdesc, &ctx->sp_ws, &ctx->sp_out, &ctx->sift_ws, &ctx->sift_pyr, &ctx->retr_ws, &ctx->retr_out, &ctx->img_ws, &ctx->orb_ws, &ctx->orb_pyr, &ctx->orb_tab};
    for (DevBuf *b : bufs) b->release();
    for (DevBuf &b : ctx->ba_ws) b.release();
    ctx->ba_loss_ws.release();
    ctx->lm_ws.release();
    ctx->tri_ws.release();
    ctx->tri_dws.release();
    ctx->fm_ws.release();
    ctx->fm_state.release();
    ctx->fm_csr.release(); ctx->fm_pairs.release();
    for (auto &kv : ctx->coords) kv.second.first.release();
    ctx->corr.release();
    ctx->corr_ws.release(); ctx->corr_hws.release(); ctx->corr_slots.release(); ctx->att_ws.release();
    if (ctx->corr_ev) (void)hipEventDestroy(ctx->corr_ev);
    ctx->lid.release(); ctx->lid_slot_off.release(); ctx->lid_hws.release(); ctx->nvt_ws.release();
    if (ctx->nvt_ev) (void)hipEventDestroy(ctx->nvt_ev);
    if (ctx->img_ev) (void)hipEventDestroy(ctx->img_ev);
    ctx->pnp_hws.release(); ctx->pnp_slots.release();
    ctx->tv_hws.release(); ctx->tv_dws.release(); ctx->tv_fws.release();
    ctx->hg_hws.release(); ctx->hg_dws.release();
    if (ctx->tv_ev) (void)hipEventDestroy(ctx->tv_ev);
    if (ctx->pnp_ev) (void)hipEventDestroy(ctx->pnp_ev);
    if (ctx->ev_made) {
        for (auto &call : ctx->ev_c)
            for (auto &row : call)
                for (auto &e : row) (void)hipEventDestroy(e);
        for (auto &row : ctx->ev_tail)
            for (auto &e : row) (void)hipEventDestroy(e);
    }
    ctx->mid_ws.release();
    if (ctx->ba_ev_made)
        { (void)hipEventDestroy(ctx->ba_pair_ev); for (auto &e : ctx->ba_tev) (void)hipEventDestroy(e); }
    if (ctx->copy_stream) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamDestroy(ctx->copy_stream);
        for (auto &e : ctx->cmp_ev) (void)hipEventDestroy(e);
        (void)hipEventDestroy(ctx->cmp_filled);
    }
    ctx->cmp_off.release(); ctx->cmp_qt[0].release(); ctx->cmp_qt[1].release();
    rcn_chol_destroy(ctx);
    if (ctx->ba_host_scal) (void)hipHostFree(ctx->ba_host_scal);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char *rcn_last_error(const rcn_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int rcn_set_stream(rcn_ctx *ctx, void *hip_stream)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
    return RCN_OK;
}

int rcn_synchronize(rcn_ctx *ctx)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipStreamSynchronize(ctx->stream));
    return RCN_OK;
}

}  // extern "C"
