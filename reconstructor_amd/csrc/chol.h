// chol.h -- host interface of the dense blocked FP64 Cholesky (K7, chol.hip): what a context keeps for it (CholState) and the
// calls of its user (ba.hip: the reduced camera system of bundle adjustment).  The schedule itself is data: chol_plan.h.
// Included by rcn_internal.h behind DevBuf; the kernels, their tile sizes and the hand-off machinery stay inside chol.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

#include "chol_plan.h"

struct rcn_ctx;

namespace chol {
constexpr int BLOCK = 128;      // block size: a system is padded to a multiple of it
}
// rhs_row: the diagonal entry under the right-hand side in row n of the padded system.  Huge, so that the row's own pivot stays positive
// whatever b' S^-1 b is; nobody reads what the factorisation leaves there.
#define RCN_RHS_BETA 1.0e200

// Everything a context keeps for the factorisation: parameters, switches, streams, events, the plan of the last shape.
struct CholState {
    chol::Params prm;                    // the schedule's parameters (chol_plan.h has the defaults and their meaning; nblk is set per plan).  Diagnostic build: RCN_CHOL_TL,
                                         // _TL_MIN, _GROUP (pair = group >= 2), _PAIR_MIN, _PIPE_MIN, _DIAG_SERVER, _WINDOW, _TL_SERIAL, _HEAD_SMALL, _FUSE_TAIL, _BULK_BEHIND, _CARVE, _PGSTREAM
    // ---- switches outside the plan
    int chain_stream_mode = 0;           // diagnostic build (RCN_CHOL_CHAIN_STREAM=1): the factorisation's chain on a highest-priority stream of the library's own
    int gate_in_kernel = 0;              // diagnostic build (RCN_CHOL_GATE_IN_KERNEL=1): waits of the small kernels off the chain inside them, not in a gate kernel in front; -1: in front on the chain too
    bool pg_prio = true;                 // diagnostic build (RCN_CHOL_PG_PRIO=0): no raised wave priority for the panel product below the head rows
    bool host_time = false;              // diagnostic build (RCN_CHOL_HOSTTIME=1): print the host time of every factorisation's enqueue
    int brk = 0;                         // diagnostic build (RCN_CHOL_BREAK): 1 = break one cross-stream hand-off (forces the one-stream fallback); 2 = and put a NaN pivot behind it
    int diag_stream_prio = 1;            // diagnostic build (RCN_DIAG_STREAM_PRIO): the resident diagonal workgroup's stream at normal priority (0) or under a CU mask of all CUs (2)
    bool safe = false;                   // a device-counter hand-off timed out once: factorise on one stream, in plain order, from then on
    bool trsv_chain = true;              // backward substitution as one launch (k_trsv_bwd_chain); off after a flag timeout
    // ---- streams
    hipStream_t aux = nullptr;           // lookahead stream: bulk trailing updates (CU mask leaves one CU per XCD to the diagonal kernel)
    hipStream_t panel = nullptr;         // second chain stream: panels and first trailing columns behind the critical tile
    hipStream_t panel2 = nullptr;        // two-level regime, plans with pg_stream only (not what ships): the panel product for the rows below the head (the bulk stream's CU mask); made on demand
    hipStream_t chain = nullptr;         // chain_stream_mode: the chain's own stream
    hipStream_t diag = nullptr;          // the resident workgroup that factors the diagonal blocks of a factorisation (k_chol_diag_server); made on demand
    std::vector<uint32_t> bulk_cu_mask;  // the bulk stream's CU mask
    hipEvent_t ev[6] = {};               // [0]: fork of the factorisation's streams, [1..4]: their joins, [5]: the chain's own stream back to the caller's
    bool prepared = false;               // rcn_chol_prepare has run
    // ---- the schedule (chol_plan.h: operations, streams, waits, tile maps) for the last shape solved; its maps in HBM
    chol::Plan plan;
    bool plan_valid = false;
    DevBuf bulk_map;
    DevBuf diag_items;                   // the resident diagonal workgroup's work list of that plan
};

// One system to factorise and solve, all pointers in HBM.  S: the padded system (lower triangle, npad = BLOCK nblk columns, identity
// below row n -- or, rhs_row, the right-hand side as row n), L: the factor's sub-diagonal tiles, Linv / SI: rcn_chol_ws, zeroed by
// the caller; flag: [0] breakdown (1) / hand-off timeout (3, 4), [12..18] the streams' counters, zero when a factorisation starts.
struct CholSystem {
    double *S, *L, *Linv, *SI;
    int *flag;
    double *rhs, *yc;                    // the right-hand side and the forward substitution's result when they do not ride in S; the solution is left in rhs
    int n, npad, nblk;
    bool rhs_row;                        // the right-hand side is row n of S and goes through the factorisation
    bool chain;                          // backward substitution as one launch (rcn_chol_bwd_one_launch)
    bool fused_finish;                   // flag words, padding and the sentinel of the one-launch substitution were written by the launch that finished S
};

struct CholWs { size_t linv, si; };      // doubles: the diagonal blocks' inverses; a super-block's inverse (both buffers)

int rcn_chol_create(rcn_ctx *ctx);       // rcn_create: streams, events and (diagnostic build) the switches from the environment
void rcn_chol_destroy(rcn_ctx *ctx);
CholWs rcn_chol_ws(const rcn_ctx *ctx, int nblk);
int rcn_chol_prepare(rcn_ctx *ctx);      // once per context: the kernels' dynamic LDS sizes
int rcn_chol_plan(rcn_ctx *ctx, int nblk);      // the schedule for nblk blocks: built once per shape and parameter set
hipStream_t rcn_chol_idle_stream(rcn_ctx *ctx);      // the panel stream: idle between factorisations (every factorisation joins its streams)
bool rcn_chol_bwd_one_launch(const rcn_ctx *ctx, int nblk);
bool rcn_chol_bwd_gave_up(rcn_ctx *ctx);        // flag 4: per-step kernels from now on; false: they were in use already
// on ctx->stream; safe: on that stream alone, in list order.  The caller reads flag[0] and decides about the fallback (CholState::safe)
hipError_t rcn_chol_factorise(rcn_ctx *ctx, const CholSystem &s, bool safe);
hipError_t rcn_chol_substitute(rcn_ctx *ctx, const CholSystem &s);      // rhs_row without (chain and fused_finish): the caller has put row n of the factor into yc
