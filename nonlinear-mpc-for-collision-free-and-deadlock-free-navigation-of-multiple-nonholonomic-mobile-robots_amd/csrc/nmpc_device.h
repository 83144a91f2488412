// nmpc_device.h — the kernel parameter block, the launch descriptors and the launcher declarations shared by nmpc_api.cpp and the three swarm
// solve kernels (nmpc_kernels.hip, nmpc_solve_lds.hip, nmpc_solve_col.hip, the latter two through nmpc_solve_common.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/nmpc.h"

// shared with the CPU oracles: NMPC_SHIFT_ESCALATION, NMPC_COLD_RETRY_ITERS, NMPC_COLD_RETRIES, NMPC_X0_TOL
#include "../../include/nmpc_constants.h"

namespace nmpc {

// f(std::integral_constant<int, M>{}) for the team size m = M in 1 .. NMPC_MAX_ROBOTS (every one is instantiated), `none` for any other m
template <int M = 1, class R, class F> R for_team_size(int m, R none, F &&f)
{
    if constexpr (M > NMPC_MAX_ROBOTS) return none;
    else return m == M ? f(std::integral_constant<int, M>{}) : for_team_size<M + 1>(m, none, f);
}

// Passed by value to every kernel (lands in SGPRs / the kernarg segment).
struct KParams {
    int32_t m, N, K, thb, nxb, nh, n_ineq, nvar, ng, rows0, rowsk, pad_rows, max_iter;
    int32_t o_ul, o_uu, o_xl, o_xu, o_pr, o_ob;     // inequality slot offsets inside one stage block
    double T, dmin2, vmax, wmax, xymax, thmax, robdim, margin, pad_value, tol, mu_init;
    double q[3], r[2];
    double rho_el;        // penalty of the elastic phase (NMPC_ELASTIC_RHO)
    union {      // the obstacle field: one of the two, chosen at compile time by the kernel instantiation (ObsField, nmpc_solve_common.h)
        double obs[3 * NMPC_MAX_OBSTACLES];      // (ox, oy, obs_r) per obstacle: the handle's config field, the same for every instance and stage
        struct {
            const double *ptr;                   // [B][S][K][3] device: per-instance field of the *_obs entry points (S = 1 or N)
            int32_t istride, sstride;            // doubles per instance (S K 3) and per stage (K 3 when S = N, 0 when S = 1)
        } ofield;
    };
    // per-instance workspace carve-up, in doubles
    int64_t stride;
    int32_t trace_inst;   // NMPC_PROFILE builds: instance whose per-iteration trace is recorded
    int32_t pairs;        // 1: pair rows present (C6:288-306); 0: multi-robot NLP without them (mpc_online_casadi_tb3_multi_centralized.py)
    const int32_t *order;       // per call: dispatch order (workgroup g solves instance order[g]) or nullptr = identity
    const int32_t *order_bad;   // device flag written by the permutation check of that order: non-zero -> the hint is ignored
    double *lam_g, *lam_x, *lam_p;      // per call (column kernel, nmpc_*_batch_duals): the multipliers of the returned point, [B][ng] / [B][nvar] / [B][2 nx], each or all nullptr
    int64_t stride2;      // workspace stride of the LDS-resident kernel (stage packs + transposed gains)
    int64_t oPACK, oKT;
    int64_t oCKPT;        // LDS-resident kernels: cost-to-go saved every NMPC_CKPT_EVERY stages of the backward sweep, WsLayout::ckpt_slots(N) slots of WsLayout::CKPT_SLOT doubles
    int64_t oELAS;        // LDS-resident kernels: elastic variables t of the pair and obstacle rows, WsLayout::el_pair + el_obs: touched only in the elastic phase
    int64_t oDUAL;        // column kernel: slacks and duals of the inequality rows (touched by the stage-parallel phases only) live here, not in LDS
    int32_t oX, oU, oLAM, oS, oZ, oDX, oDU, oLAMN, oDS, oDZ, oSN, oCS, oC, oH, oGX, oHUU, oGU, oHVT, oHTT, oKG, oKFF, oCKP, oEL;      // oCKP: the HBM-resident kernel's saved cost-to-go, [(N-1)/NMPC_CKPT_EVERY + 1][HbmWs::ckpt_slot]; oEL: its elastic variables and their steps, 2 x HbmWs::el_half
};

// The two places where the HBM-resident kernel's workspace (carved up by fill_params, the offsets above) has structure inside an array
struct HbmWs {
    static constexpr int ckpt_slot(int nx) { return nx * nx + nx; }                       // oCKP: one slot holds the saved cost-to-go [P | p]
    static constexpr int64_t el_half(int N, int nh) { return (int64_t)(N + 1) * nh; }     // oEL: the elastic variables t, one per inequality slot, then their steps
};

// The pose reference of the cost as eval_kernel and kkt_residual_kernel read it, sum_k (X_k - xs_k)' Q (X_k - xs_k): instance b's rows start at
// ptr + b * istride and stage k reads row k * sstride.  The plain calls point it at the xs half of p (ptr = p + n_x, istride = 2 n_x, sstride = 0),
// the *_ref calls at ref [B][S][n_x] (istride = S n_x; sstride = n_x when S = N, else 0).  A kernel argument of its own: KParams, which the solve
// kernels share, keeps its layout.  The column kernel's tracking instantiations (track_col_kernel, nmpc_solve_batch_ref) read the same struct
// through PoseRows (nmpc_solve_common.h).
struct PoseRef {
    const double *ptr;
    int32_t istride, sstride;
};

// The solve kernels by the code nmpc_options_t.kernel pins and NMPC_QUERY_KERNEL_FOR_BATCH answers (include/nmpc.h), and the shapes of the
// column kernel: one, two or four wavefronts per instance.  KERN_COL_LAT is the column kernel in one of its two latency shapes.
enum { KERN_HBM = 1, KERN_LDS = 2, KERN_COL = 3, KERN_COL_LAT = 4 };
enum { SHAPE_TP = 0, SHAPE_LAT2 = 1, SHAPE_LAT4 = 2 };

// The instantiation one launch runs: the template arguments of solve_kernel<M, TPB> (kernel 1), solve_lds_kernel<M, THB, TPB> (2) or
// solve_col_kernel<M, THB, DL, TPB> (3), and its dynamic LDS.  Filled by the select_* function of each kernel; its launcher launches exactly
// this instantiation (hipErrorInvalidValue where it does not exist) and selects nothing itself.
struct SolveVariant {
    int kernel, m, thb, flags, threads;      // kernel: KERN_HBM / KERN_LDS / KERN_COL; thb: 0 for kernel 1 (no such template argument); flags: DL of the column kernel (bit 2: per-instance obstacle field), bit 3 (8): track_col_kernel<M, THB, DL, TPB> with DL = flags - 8; else 0
    size_t lds;
};
// false: team size not instantiated
bool select_solve(const KParams &P, int m, int B, SolveVariant *v);
bool select_solve_lds(const KParams &P, int m, int B, SolveVariant *v);
bool select_solve_col(const KParams &P, int m, int shape, bool ofield, SolveVariant *v);      // shape: SHAPE_*; ofield: the per-instance obstacle field P.ofield
bool select_track_col(const KParams &P, int m, int shape, SolveVariant *v);      // the tracking kernel (always with P.ofield): flags carry bit 3

// device pointers of one solve call: inputs, outputs (each of obj .. kkt may be nullptr), the handle's workspace and profile counters
struct SolveArgs {
    const double *p, *w0;
    double *w_out, *obj;
    int32_t *status, *iters;
    double *kkt, *ws;
    long long *prof;
    PoseRef ref;      // the tracking kernel's launches only: the per-stage pose reference of the call
};
hipError_t launch_solve(const KParams &P, const SolveVariant &v, int B, const SolveArgs &a, hipStream_t st);
hipError_t launch_solve_lds(const KParams &P, const SolveVariant &v, int B, const SolveArgs &a, hipStream_t st);
hipError_t launch_solve_col(const KParams &P, const SolveVariant &v, int B, const SolveArgs &a, hipStream_t st);
size_t lds_kernel_bytes(const KParams &P, int m);                 // the element-per-lane kernel's throughput shape
size_t col_kernel_bytes(const KParams &P, int m, int shape);      // = select_solve_col(..).lds
void lds_workspace_fill(KParams *P, int m);                       // the LDS-resident kernels' workspace: oPACK, oKT, oDUAL, oCKPT, oELAS and stride2 from WsLayout (nmpc_solve_common.h); m not supported: all 0
hipError_t launch_eval(const KParams &P, const PoseRef &xr, int m, int B, const double *p, const double *w, double *f, double *g, hipStream_t st, bool ofield = false);      // ofield: P.ofield is the obstacle field
// KKT residuals of (w, lam_g, lam_x): res [B][6] = (stat, eq, ineq, bnd, compl, sign), grad_lag [B][nvar] or nullptr (include/nmpc.h, nmpc_kkt_batch)
hipError_t launch_kkt(const KParams &P, const PoseRef &xr, int m, int B, const double *p, const double *w, const double *lam_g, const double *lam_x, double *res, double *grad_lag,
                      hipStream_t st, bool ofield);
constexpr int NMPC_SENS_OBS = 16;      // the sensitivity kernels' MS = team size + NMPC_SENS_OBS * (per-instance obstacle field), as eval_kernel's NMPC_EVAL_OBS
// plan sensitivities of (w, lam_g, lam_x) (include/nmpc.h, nmpc_sens_batch; nmpc_sens.hip): dw [B][nvar] for dp [B][2 nx] (both or neither), gains [B][gain_stages][nu][nx] or
// nullptr, info [B]; ws: the workspace of a handle that runs on the column kernel (its pivot-row region holds [G_k | g_k] between the two passes)
hipError_t launch_sens(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, double *dw, double *gains,
                       int gain_stages, int32_t *info, double *ws, hipStream_t st, bool ofield);
// the transposes of the same maps applied to wbar [B][nvar] (include/nmpc.h, nmpc_sens_adjoint_batch; nmpc_sens.hip): pbar [B][2 nx] and
// obsbar [B][obs_stages][K][3], each or both nullptr (obsbar only with ofield); info and ws as launch_sens
hipError_t launch_sens_adjoint(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *wbar, double *pbar,
                               double *obsbar, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield);
// the forward plan update (include/nmpc.h, nmpc_sens_update_batch; nmpc_sens.hip): dw [B][nvar] and alpha [B], each or both nullptr, for
// dp [B][2 nx], dobs [B][obs_stages][K][3] (only with ofield) and rhs [B][nvar], each nullptr for zero; info and ws as launch_sens
hipError_t launch_sens_fwd(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                           const double *rhs, double *dw, double *alpha, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield);
// the multiplier updates of the forward plan update (include/nmpc.h, nmpc_sens_update_batch_duals; nmpc_sens_dual.hip), launched behind launch_sens_fwd on its
// stream: from that call's inputs, its dw [B][nvar] and its verdicts info [B], dlam_g [B][ng], dlam_x [B][nvar] and alpha_dual [B], each nullptr or written; no workspace
hipError_t launch_sens_dual(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, const double *dw, int obs_stages, const int32_t *info, double *dlam_g, double *dlam_x, double *alpha_dual,
                            hipStream_t st, bool ofield);
// the forward plan update for D directions (include/nmpc.h, nmpc_sens_update_batch_multi; nmpc_sens_multi.hip): dw [B][D][nvar] (required) and alpha [B][D]
// or nullptr for dp [B][D][2 nx], dobs [B][D][obs_stages][K][3] (only with ofield) and rhs [B][D][nvar], each nullptr for zero; 1 <= D <= NMPC_SENS_MAX_DIRS;
// info [B] and ws as launch_sens.  plan_dirs_per_pass: the directions one pass of the recursion carries for team size m (NMPC_QUERY_SENS_DIRS_PER_PASS)
hipError_t launch_plan_dirs(const KParams &P, int m, int B, int D, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, double *dw, double *alpha, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield);
int plan_dirs_per_pass(int m);
// the multiplier updates of the D directions (include/nmpc.h, nmpc_sens_update_batch_multi_duals; nmpc_sens_dual_multi.hip), launched behind launch_plan_dirs on
// its stream: from that call's inputs, its dw [B][D][nvar] and its verdicts info [B], dlam_g [B][D][ng], dlam_x [B][D][nvar], dlam_p [B][D][2 nx] and
// alpha_dual [B][D], each nullptr or written; no workspace
hipError_t launch_dual_dirs(const KParams &P, int m, int B, int D, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, const double *dw, int obs_stages, const int32_t *info, double *dlam_g, double *dlam_x, double *dlam_p,
                            double *alpha_dual, hipStream_t st, bool ofield);
hipError_t launch_shift(const KParams &P, int m, int B, const double *p, const double *w_in, double *w_next, double *x0n, int x0_stride, const int32_t *keep_status, hipStream_t st);      // x0_stride: doubles between the x0_next rows (0 = n_x); keep_status: instances with status 2 / 3 there are left untouched (or nullptr)
hipError_t launch_order_by_iters(int B, const int32_t *iters, int32_t *order, hipStream_t st);
hipError_t launch_odometry(long n, const double *odom, const double *init, double *pose, int wrap, hipStream_t st);
hipError_t launch_order_check(int B, const int32_t *order, int32_t *count, int32_t *bad, hipStream_t st);

}  // namespace nmpc
