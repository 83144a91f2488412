// nmpc_sens.hip — the three calls that solve the linearisation of the solver's barrier KKT system at a given primal-dual point (w, lam_g, lam_x)
// by one backward stage recursion and one forward pass per instance (include/nmpc.h), as the three kinds of one kernel, sens_kernel<MS, KIND>:
//   SENS_PLAN     nmpc_sens_batch: plan sensitivities dw = S_p dp and the feedback gains.  Affine column -2 Q dxs on X_k (k < N), p_N = 0;
//                 forward pass from dX_0 = dx0, stored to dw.
//   SENS_ADJOINT  nmpc_sens_adjoint_batch: pbar = S_p' wbar and obsbar = S_o' wbar for a cotangent wbar of the plan.  The KKT matrix of the
//                 linearisation is symmetric, so the adjoint is the same recursion with a general affine column — -wbar on U_k and X_k,
//                 p_N = -wbar_{X_N} — and a forward pass from v_{X_0} = 0 that stores nothing of v: it contracts v with 2 Q (the goal) and with
//                 the obstacle blocks M_o of stages 1 .. N-1 (the field), and takes the measured state's part from the affine cost-to-go of stage 0.
//   SENS_UPDATE   nmpc_sens_update_batch: dw = S_p dp + S_o dobs (+ the general linear term rhs) in one launch, and the step limit alpha: how
//                 much of (dw, dobs) keeps every linearised slack non-negative.  dw minimises 1/2 dw' W dw + c' dw on dX_0 = dx0 and the
//                 linearised defects, c = -2 Q dxs on X_k (k < N) - rhs + M_o dobs; the forward pass of SENS_PLAN, which here also walks the alpha
//                 items of every stage.
//
// One wavefront per instance.  Lane j owns column j of the augmented stage matrix [F | f] in the order [U_k; X_k | affine], n_u + n_x + 1 <= 51
// columns, which is assembled in LDS (ten robots: 20 KB) and eliminated in registers; the cost-to-go [P_{k+1} | p_{k+1}] stays in LDS between
// stages.  A lane writes its own column only; what it needs of another column — an entry of P in the assembly, a multiplier of the
// elimination — it reads after an LDS fence or from the other lane's register.  [B A] has at most three entries per column (per-robot 3 x 3 / 3 x 2 blocks), so [B A]' P [B A] is a
// three-term gather per entry and three row operations per robot.  The terms of W_k are restated from the formulas of include/nmpc.h, with the
// row and multiplier indexing of kkt_residual_kernel (nmpc_kernels.hip); the obstacle entry of stage k comes through ObsField.
// [G_k | g_k] of every stage goes to the pivot-row region [N][KTS] of the handle's workspace (WsLayout, nmpc_solve_common.h), which is idle
// between the handle's calls and which every solve writes before it reads; the forward pass reads it back.  No solve kernel is involved.
//
// The stage recursion and the forward state propagation are stated once, in the kernel body; what a kind does differently stands in place under
// `if constexpr (KIND == ...)`.  Nothing of the two loops is behind a function boundary: with the loop body, its assembly or its elimination in an
// inlined device function the six-robot kernel leaves the 168 registers that still give three waves per SIMD, and nine and ten robots go from two
// waves to one (tests/test_sens_occupancy_host.py holds every instantiation to its waves per SIMD).  A term of W_k lives in
// two places: here and, as a matrix-vector product, in nmpc_sens_dual.hip — a change to one belongs in both; the parity tables
// (tests/sens_points.py) hold each kind and the dual kernel against its own numpy reference.
// Sums run in a fixed order inside the wavefront — the terms of c at one entry: goal, rhs, then the obstacles in index order; robots that share an
// obstacle in index order; stages that share an entry in stage order; alpha is one wave-wide minimum — no atomics, the same inputs give the same bits.
#include "nmpc_solve_common.h"

namespace nmpc {

// v of lane `lane` (a literal after unrolling), for every lane
__device__ __forceinline__ double lane_f64(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

constexpr int SENS_PLAN = 0, SENS_ADJOINT = 1, SENS_UPDATE = 2;      // KIND of sens_kernel

// The parameters are the union of the three calls' pointers, those of another kind nullptr and never read, and S: gain_stages of SENS_PLAN (1 or N),
// obs_stages of the other two (1 or N; read only with obsbar / dobs).  They are kernel parameters, each __restrict__, and not members of one struct
// passed by value: the qualifier means nothing on a struct member or on a local copy of one, and without it the plan kind of three robots and more
// takes a private segment of 36 bytes that the three separate kernels did not have.
template <int MS, int KIND>
__global__ __launch_bounds__(64) void sens_kernel(const KParams P, const double *__restrict__ w, const double *__restrict__ lam_g, const double *__restrict__ lam_x,
                                                  const double *__restrict__ dp, const double *__restrict__ wbar, const double *__restrict__ dobs,
                                                  const double *__restrict__ rhs, double *__restrict__ dw, double *__restrict__ gains, double *__restrict__ pbar,
                                                  double *__restrict__ obsbar, double *__restrict__ alpha, int S, int32_t *__restrict__ info, double *__restrict__ ws)
{
    constexpr int M_ = MS % NMPC_SENS_OBS, OS = MS / NMPC_SENS_OBS;
    using G = G2<M_, 0>;
    constexpr int NX = G::NX, NU = G::NU, NZ = G::NZ, NP = G::NP;
    constexpr int LDF = NZ + 1, LDP = NX + 1, LDG = NX + 1;      // row strides of [F | f], [P | p] and, in the workspace, [G_k | g_k]
    static_assert(NZ + 1 <= 64, "one lane per column of the augmented stage matrix");
    static_assert(NU * LDG <= G::KTS, "[G_k | g_k] fits the stage's pivot-row slot of the workspace");
    static_assert(3 * NMPC_MAX_OBSTACLES <= 64, "one lane per entry of a stage's obstacle cotangent");
    static_assert(NP <= 64, "one lane per pair row of a stage");
    __shared__ double F[NZ * LDF], Pb[NX * LDP], xk[NX], uk[NU], lx[NZ], lk[NX + NP + M_ * NMPC_MAX_OBSTACLES], cs[3 * M_], qx[NX], qu[NU], dx[NX], du[NU];      // qu: not SENS_PLAN, which does not pay for it
    const int j = threadIdx.x, N = P.N, K = P.K;
    const size_t b = blockIdx.x;
    const double *X = w + b * P.nvar, *U = X + (size_t)(N + 1) * NX;
    const double *lg = lam_g + b * P.ng, *lxX = lam_x + b * P.nvar, *lxU = lxX + (size_t)(N + 1) * NX;
    const double *wbX = KIND == SENS_ADJOINT ? wbar + b * P.nvar : nullptr, *wbU = KIND == SENS_ADJOINT ? wbX + (size_t)(N + 1) * NX : nullptr;
    const double *rhX = (KIND == SENS_UPDATE && rhs) ? rhs + b * P.nvar : nullptr, *rhU = rhX ? rhX + (size_t)(N + 1) * NX : nullptr;
    const int nob = 3 * K;      // entries of one stage of dobs / of the obstacle cotangent: there lane j < nob owns component j % 3 of obstacle j / 3
    const double *dob = (KIND == SENS_UPDATE && dobs) ? dobs + b * (size_t)S * nob : nullptr;
    double *kt = ws + b * P.stride2 + P.oKT;                     // [N][KTS], of which [NU][LDG] per stage are used here
    const ObsField<OS> OB(P, b);
    const int npairs = P.pairs ? NP : 0;
    const double T = P.T;
    // the variable of this lane's column: control (rob, comp: 0 v, 1 omega), state (rob, comp: 0 x, 1 y, 2 theta) or the affine column
    const bool isu = j < NU, isx = j >= NU && j < NZ, col = j <= NZ;
    const int rob = isu ? j / 2 : (isx ? (j - NU) / 3 : 0), comp = isu ? j % 2 : (isx ? (j - NU) % 3 : 0);
    bool bad = false, indef = false;
    // a variable -ub <= v <= ub with multiplier l: max(l, 0) / (ub - v) + max(-l, 0) / (v + ub); a positive multiplier on s <= 0 is info 2
    auto bterm = [&](double l, double v, double ub) -> double {
        double t = 0.0;
        if (ub < INFINITY) {
            const double s = l > 0.0 ? ub - v : v + ub, z = fabs(l);
            if (l > 0.0 || l < 0.0) { if (s <= 0.0) bad = true; else t = z / s; }
        }
        return t;
    };
    // an inequality row g >= lb with multiplier l and slack s = g - lb: Sigma = max(-l, 0) / s
    auto sigma = [&](double l, double s) -> double {
        double t = 0.0;
        if (-l > 0.0) { if (s <= 0.0) bad = true; else t = -l / s; }
        return t;
    };
    const double thub = P.thb ? P.thmax : INFINITY;

    // the goal's part of the linear term, -2 Q dxs on every X_k, k < N: all of it for SENS_PLAN, the first term of c for SENS_UPDATE; the adjoint's
    // linear term is -wbar, loaded stage by stage below.  P_N = the bound terms of X_N, p_N = 0, -wbar_{X_N} or -rhs_{X_N}
    double qgoal = 0.0;
    if constexpr (KIND == SENS_PLAN) {
        if (j < NX) qx[j] = dp ? -2.0 * P.q[j % 3] * dp[b * 2 * NX + NX + j] : 0.0;
    }
    if constexpr (KIND == SENS_UPDATE) qgoal = (dp && j < NX) ? -2.0 * P.q[j % 3] * dp[b * 2 * NX + NX + j] : 0.0;
    if (j <= NX)
        for (int r = 0; r < NX; r++) {
            if constexpr (KIND == SENS_PLAN) Pb[r * LDP + j] = 0.0;
            if constexpr (KIND == SENS_ADJOINT) Pb[r * LDP + j] = j == NX ? -wbX[(size_t)N * NX + r] : 0.0;
            if constexpr (KIND == SENS_UPDATE) Pb[r * LDP + j] = (j == NX && rhX) ? -rhX[(size_t)N * NX + r] : 0.0;
        }
    if (j < NX) Pb[j * LDP + j] = bterm(lxX[(size_t)N * NX + j], X[(size_t)N * NX + j], (j % 3 == 2) ? thub : P.xymax);
    lds_sync<64>();

#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
        // ---- the stage's point and multipliers: X_k, U_k, lam_x of both (X_0 carries none), lam_g of the stage block (defect, pair, obstacle rows)
        const double *lgk = lg + P.rows0 + (size_t)k * P.rowsk;
        if (j < NX) xk[j] = X[(size_t)k * NX + j];
        if (j < NU) uk[j] = U[(size_t)k * NU + j];
        if (j < NZ) lx[j] = isu ? lxU[(size_t)k * NU + j] : (k > 0 ? lxX[(size_t)k * NX + j - NU] : 0.0);
        if constexpr (KIND == SENS_ADJOINT) {
            if (j < NX) qx[j] = -wbX[(size_t)k * NX + j];
            if (j < NU) qu[j] = -wbU[(size_t)k * NU + j];
        }
        for (int e = j; e < P.rowsk; e += 64) lk[e] = lgk[e];
        if constexpr (KIND == SENS_UPDATE) {
            // ---- the linear term c of the stage: lane j < NX forms entry j of X_k — the goal, then rhs, then (M_o dobs) of the robot's obstacle
            //      rows in index order, by the block formulas of the adjoint's contraction below (include/nmpc.h) with the slack rounded as
            //      there; stage 0 carries no obstacle term
            if (j < NX) {
                double q = qgoal;
                if (rhX) q -= rhX[(size_t)k * NX + j];
                if (dob && k > 0 && j % 3 < 2) {
                    const int i = j / 3, oc = j % 3;
                    const double xi = X[(size_t)k * NX + 3 * i], yi = X[(size_t)k * NX + 3 * i + 1];
                    const double *d = dob + (S == N ? k : 0) * nob;
                    for (int o = 0; o < K; o++) {
                        const double l = lgk[NX + npairs + i * K + o];
                        const double ex = xi - OB(k, o, 0), ey = yi - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey), n0 = ex / rr, n1 = ey / rr, nc = oc ? n1 : n0;
                        const double sg = -l > 0.0 ? -l / (rr - P.robdim - OB(k, o, 2) - P.margin) : 0.0;      // s <= 0 here is verdict 2 of the assembly below
                        const double d0 = d[3 * o], d1 = d[3 * o + 1], nd = n0 * d0 + n1 * d1;
                        q -= l * ((oc ? d1 : d0) - nc * nd) / rr + sg * nc * nd + sg * nc * d[3 * o + 2];
                    }
                }
                qx[j] = q;
            }
            if (j < NU) qu[j] = rhU ? -rhU[(size_t)k * NU + j] : 0.0;
        }
        lds_sync<64>();
        if (j < M_) {
            double s, c;
            sincos(xk[3 * j + 2], &s, &c);
            cs[3 * j] = c; cs[3 * j + 1] = s; cs[3 * j + 2] = T * uk[2 * j];
        }
        lds_sync<64>();
        if (col) {
            // ---- [B A]' [P | p] [B A | e]: this lane's column of [B A | e] has the entries (r0, c0), (r1, c1), (r2, c2) —
            //      v_i: T cos, T sin on (x_i, y_i); omega_i: T on theta_i; x_i, y_i: 1; theta_i: 1 and -T v sin, T v cos on (x_i, y_i); affine: p itself
            const double c_ = cs[3 * rob], s_ = cs[3 * rob + 1], tv = cs[3 * rob + 2];
            int r0 = NX, r1 = 0, r2 = 0;
            double c0 = 1.0, c1 = 0.0, c2 = 0.0;
            if (isu) {
                if (comp == 0) { r0 = 3 * rob; c0 = T * c_; r1 = 3 * rob + 1; c1 = T * s_; }
                else { r0 = 3 * rob + 2; c0 = T; }
            } else if (isx) {
                r0 = j - NU;
                if (comp == 2) { r1 = 3 * rob; c1 = -tv * s_; r2 = 3 * rob + 1; c2 = tv * c_; }
            }
            for (int r = 0; r < NX; r++) F[(NU + r) * LDF + j] = c0 * Pb[r * LDP + r0] + c1 * Pb[r * LDP + r1] + c2 * Pb[r * LDP + r2];
            //      ... then the rows: the control rows from the state rows, and the heading rows take their two position terms
            for (int i = 0; i < M_; i++) {
                const double a0 = F[(NU + 3 * i) * LDF + j], a1 = F[(NU + 3 * i + 1) * LDF + j], a2 = F[(NU + 3 * i + 2) * LDF + j];
                const double ci = cs[3 * i], si = cs[3 * i + 1], tvi = cs[3 * i + 2];
                F[(2 * i) * LDF + j] = T * (ci * a0 + si * a1);
                F[(2 * i + 1) * LDF + j] = T * a2;
                F[(NU + 3 * i + 2) * LDF + j] = a2 + tvi * (ci * a1 - si * a0);
            }
            // ---- + W_k, this lane's column: 2 R, 2 Q, the heading / speed curvature of the defects, the bound terms, the pair and obstacle blocks
            const double l0 = lk[3 * rob], l1 = lk[3 * rob + 1];
            const double cross = T * (l0 * s_ - l1 * c_);      // d2 L / d theta_i d v_i
            if (isu) {
                F[j * LDF + j] += 2.0 * P.r[comp] + bterm(lx[j], uk[j], comp ? P.wmax : P.vmax);
                if (comp == 0) F[(NU + 3 * rob + 2) * LDF + j] += cross;
            } else if (isx) {
                double dg = 2.0 * P.q[comp];
                if (k > 0) dg += bterm(lx[j], xk[j - NU], comp == 2 ? thub : P.xymax);
                if (comp == 2) { dg += tv * (l0 * c_ + l1 * s_); F[(2 * rob) * LDF + j] += cross; }
                F[j * LDF + j] += dg;
                if (comp < 2 && k > 0) {      // the pair and obstacle rows of stages 1 .. N-1 (those of stage 0 act on the pinned X_0: nothing)
                    const double xi = xk[3 * rob], yi = xk[3 * rob + 1];
                    double *own = &F[(NU + 3 * rob) * LDF + j];      // rows (x_i, y_i) of this column
                    for (int a = 0; a < (npairs ? M_ : 0); a++) {
                        if (a == rob) continue;
                        const double l = lk[NX + pidx_any<M_>(rob, a)];
                        const double ex = xi - xk[3 * a], ey = yi - xk[3 * a + 1], ed = comp ? ey : ex;
                        const double sg = 4.0 * sigma(l, ex * ex + ey * ey - P.dmin2);      // grad g = 2 (e, -e) on (robot i, robot a)
                        const double t0 = sg * ed * ex + (comp == 0 ? 2.0 * l : 0.0), t1 = sg * ed * ey + (comp == 1 ? 2.0 * l : 0.0);
                        own[0] += t0; own[LDF] += t1;
                        F[(NU + 3 * a) * LDF + j] -= t0; F[(NU + 3 * a + 1) * LDF + j] -= t1;
                    }
                    for (int o = 0; o < K; o++) {
                        const double l = lk[NX + npairs + rob * K + o];
                        const double ex = xi - OB(k, o, 0), ey = yi - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey), n0 = ex / rr, n1 = ey / rr, nd = comp ? n1 : n0;
                        const double sg = sigma(l, rr - P.robdim - OB(k, o, 2) - P.margin);      // grad g = n; Hessian (I - n n') / r
                        own[0] += l * ((comp == 0 ? 1.0 : 0.0) - n0 * nd) / rr + sg * n0 * nd;
                        own[LDF] += l * ((comp == 1 ? 1.0 : 0.0) - n1 * nd) / rr + sg * n1 * nd;
                    }
                }
            } else {
                if constexpr (KIND != SENS_PLAN)
                    for (int e = 0; e < NU; e++) F[e * LDF + j] += qu[e];
                for (int e = 0; e < NX; e++) F[(NU + e) * LDF + j] += qx[e];
            }
        }
        lds_sync<64>();
        if (indef) continue;      // a pivot <= 0 further down the horizon: only the slacks of the remaining stages are still looked at (info 2)
        // ---- the lane takes its column into registers and eliminates the n_u pivots there: the multiplier of row r is entry r of the pivot's
        //      column, read from the pivot's lane (fully unrolled: every register index and lane number is a literal)
        double c[NZ];
        const int jc = col ? j : 0;      // lanes without a column carry a copy of column 0 that nothing reads
#pragma unroll
        for (int r = 0; r < NZ; r++) c[r] = F[r * LDF + jc];
#pragma unroll
        for (int i = 0; i < NU; i++) {
            const double d = lane_f64(c[i], i);
            if (!(d > 0.0)) indef = true;
            const bool upd = j > i;
            const double rd = 1.0 / d, pj = c[i];
#pragma unroll
            for (int r = i + 1; r < NZ; r++) {
                const double m = lane_f64(c[r], i) * rd;      // lane i itself is not updated in its own step
                c[r] = upd ? c[r] - m * pj : c[r];
            }
        }
        if (indef) continue;
        // ---- [G_k | g_k] = -F_uu^-1 [F_ux | f_u] by back-substitution in the state and affine columns (entry (i, l) of the factor: register i of
        //      lane l), then out; [P_k | p_k] for the next stage
#pragma unroll
        for (int i = NU - 1; i >= 0; i--) {
            double acc = c[i];
#pragma unroll
            for (int l = i + 1; l < NU; l++) acc += lane_f64(c[i], l) * c[l];
            const double gi = -acc / lane_f64(c[i], i);
            c[i] = isu ? c[i] : gi;
        }
        if (col && !isu) {
            if constexpr (KIND == SENS_PLAN) {
                if (gains && isx && (S == N || k == 0)) {
                    double *g = gains + ((b * S + (S == N ? k : 0)) * NU) * NX + (j - NU);
#pragma unroll
                    for (int i = 0; i < NU; i++) g[i * NX] = c[i];
                }
            }
            // [G_k | g_k] for the forward pass, where the call has one: with dw, always (the adjoint), with dw or alpha
            if (KIND == SENS_PLAN ? dw != nullptr : (KIND == SENS_ADJOINT || dw || alpha)) {
#pragma unroll
                for (int i = 0; i < NU; i++) kt[(size_t)k * G::KTS + i * LDG + (j - NU)] = c[i];
            }
#pragma unroll
            for (int r = 0; r < NX; r++) Pb[r * LDP + (j - NU)] = c[NU + r];
        }
        lds_sync<64>();
    }

    const int verdict = __ballot(bad) != 0 ? 2 : (indef ? 1 : 0);
    if (j == 0) info[b] = verdict;
    if (verdict != 0) {      // no strict minimiser of the barrier problem, or no interior point: the instance's outputs are zeros, and no step at all
        if constexpr (KIND == SENS_PLAN) {
            if (gains)
                for (int e = j; e < S * NU * NX; e += 64) gains[b * S * NU * NX + e] = 0.0;
        }
        if constexpr (KIND == SENS_ADJOINT) {
            if (pbar)
                for (int e = j; e < 2 * NX; e += 64) pbar[b * 2 * NX + e] = 0.0;
            if (obsbar)
                for (int e = j; e < S * nob; e += 64) obsbar[b * S * nob + e] = 0.0;
        } else {
            if (dw)
                for (int e = j; e < P.nvar; e += 64) dw[b * P.nvar + e] = 0.0;
        }
        if constexpr (KIND == SENS_UPDATE) {
            if (alpha && j == 0) alpha[b] = 0.0;
        }
        return;
    }
    if (KIND == SENS_PLAN ? !dw : KIND == SENS_ADJOINT ? (!pbar && !obsbar) : (!dw && !alpha)) return;
    if constexpr (KIND == SENS_ADJOINT) {
        // pbar_x0: the multiplier of the adjoint QP's initial block, minus the affine part p_0 of the stage-0 cost-to-go (<pbar, dp> = <wbar, S_p dp>)
        if (pbar && j < NX) pbar[b * 2 * NX + j] = -Pb[j * LDP + NX];
    }
    // ---- forward pass from v_{X_0} = dx0 (the adjoint: 0): v_{U_k} = G_k v_{X_k} + g_k, v_{X_{k+1}} = A_k v_{X_k} + B_k v_{U_k}.  SENS_PLAN and
    //      SENS_UPDATE store v to dw; the update's walk also takes the alpha items of the stage it stands on: the smallest s / (-ds) over the items
    //      with s > 0 and ds < 0, a lane's own minimum first.  The adjoint stores nothing of v: it keeps sum_k 2 Q v_{X_k} (pbar_xs) and, at stages
    //      1 .. N-1, -M_o' v: v_{X_k} against the obstacle blocks of the stage
    __syncthreads();      // the rows of [G_k | g_k] were written by other lanes
    double *dX = (KIND != SENS_ADJOINT && dw) ? dw + b * P.nvar : nullptr, *dU = dX ? dX + (size_t)(N + 1) * NX : nullptr;
    double xsum = 0.0, osum = 0.0;      // the adjoint's sums
    double amin = 1.0;                  // the update's step limit
    auto item = [&](double s, double ds) { if (s > 0.0 && ds < 0.0) amin = fmin(amin, s / -ds); };
    // both sides of the bound -ub <= v <= ub along dv: upper s = ub - v, ds = -dv; lower s = v + ub, ds = dv
    auto bound = [&](double v, double dv, double ub) { if (ub < INFINITY) { item(ub - v, -dv); item(v + ub, dv); } };
    if (j < NX) dx[j] = (KIND == SENS_PLAN || (KIND == SENS_UPDATE && dp)) ? dp[b * 2 * NX + j] : 0.0;
    lds_sync<64>();
#pragma unroll 1
    for (int k = 0; k < N; k++) {
        if constexpr (KIND == SENS_ADJOINT) {
            if (j < NX) xsum += 2.0 * P.q[j % 3] * dx[j];
            if (obsbar && j < nob) {
                // robots that share the obstacle are summed in index order, stages that share an entry (S == 1) in stage order
                const int o = j / 3, oc = j % 3;
                double t = 0.0;
                if (k > 0) {
                    const double *lgo = lg + P.rows0 + (size_t)k * P.rowsk + NX + npairs + o;
                    const double ox = OB(k, o, 0), oy = OB(k, o, 1), orad = OB(k, o, 2);
                    for (int i = 0; i < M_; i++) {
                        const double l = lgo[i * K];
                        const double ex = X[(size_t)k * NX + 3 * i] - ox, ey = X[(size_t)k * NX + 3 * i + 1] - oy, rr = sqrt(ex * ex + ey * ey);
                        const double n0 = ex / rr, n1 = ey / rr, v0 = dx[3 * i], v1 = dx[3 * i + 1], nv = n0 * v0 + n1 * v1;
                        const double sg = -l > 0.0 ? -l / (rr - P.robdim - orad - P.margin) : 0.0;      // the slack as the backward pass rounds it; positive: verdict 0
                        t += oc == 2 ? sg * nv : l * ((oc ? v1 : v0) - (oc ? n1 : n0) * nv) / rr + sg * (oc ? n1 : n0) * nv;
                    }
                }
                if (S == N) obsbar[(b * S + k) * nob + j] = t;
                else osum += t;
            }
        }
        if ((KIND == SENS_PLAN || dX) && j < NX) dX[(size_t)k * NX + j] = dx[j];
        if (j < NU) {
            const double *g = kt + (size_t)k * G::KTS + j * LDG;
            double u = g[NX];
            for (int c = 0; c < NX; c++) u += g[c] * dx[c];
            du[j] = u;
            if (KIND == SENS_PLAN || dU) dU[(size_t)k * NU + j] = u;
            if constexpr (KIND == SENS_UPDATE) {
                if (alpha) bound(U[(size_t)k * NU + j], u, (j & 1) ? P.wmax : P.vmax);
            }
        }
        if constexpr (KIND == SENS_UPDATE) {
            if (alpha && k > 0) {
                // the bounds of X_k on the lanes that own its entries, the pair rows on lanes j < NP, the obstacle rows (robot e / K, obstacle e % K) in a loop
                const double *Xk = X + (size_t)k * NX;
                if (j < NX) bound(Xk[j], dx[j], (j % 3 == 2) ? thub : P.xymax);
                if (j < npairs) {
                    int i = 0, a = 0;
                    pair_of<M_>(j, i, a);
                    const double ex = Xk[3 * i] - Xk[3 * a], ey = Xk[3 * i + 1] - Xk[3 * a + 1];
                    item(ex * ex + ey * ey - P.dmin2, 2.0 * (ex * (dx[3 * i] - dx[3 * a]) + ey * (dx[3 * i + 1] - dx[3 * a + 1])));
                }
                const double *d = dob ? dob + (S == N ? k : 0) * nob : nullptr;
                for (int e = j; e < M_ * K; e += 64) {
                    const int i = e / K, o = e % K;
                    const double orad = OB(k, o, 2);
                    const double ex = Xk[3 * i] - OB(k, o, 0), ey = Xk[3 * i + 1] - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey), n0 = ex / rr, n1 = ey / rr;
                    const double d0 = d ? d[3 * o] : 0.0, d1 = d ? d[3 * o + 1] : 0.0, d2 = d ? d[3 * o + 2] : 0.0;
                    item(rr - P.robdim - orad - P.margin, n0 * (dx[3 * i] - d0) + n1 * (dx[3 * i + 1] - d1) - d2);
                }
            }
        }
        lds_sync<64>();
        double xn = 0.0;
        if (j < NX) {
            const int r = j / 3, d = j % 3;
            const double v = U[(size_t)k * NU + 2 * r];
            double s, c;
            sincos(X[(size_t)k * NX + 3 * r + 2], &s, &c);
            xn = d == 0 ? dx[j] + T * (c * du[2 * r] - v * s * dx[3 * r + 2])
                 : d == 1 ? dx[j] + T * (s * du[2 * r] + v * c * dx[3 * r + 2])
                          : dx[j] + T * du[2 * r + 1];
        }
        lds_sync<64>();
        if (j < NX) dx[j] = xn;
        lds_sync<64>();
    }
    if constexpr (KIND == SENS_ADJOINT) {
        if (pbar && j < NX) pbar[b * 2 * NX + NX + j] = xsum;
        if (obsbar && S != N && j < nob) obsbar[b * nob + j] = osum;
    } else {
        if ((KIND == SENS_PLAN || dX) && j < NX) dX[(size_t)N * NX + j] = dx[j];
    }
    if constexpr (KIND == SENS_UPDATE) {
        if (alpha) {
            if (j < NX) bound(X[(size_t)N * NX + j], dx[j], (j % 3 == 2) ? thub : P.xymax);
            const double a = wave_min(amin);
            if (j == 0) alpha[b] = a;
        }
    }
}

// one launch: the kernel of the team size, with or without the per-instance obstacle field
template <int KIND> static hipError_t launch_sens_kind(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp,
                                                       const double *wbar, const double *dobs, const double *rhs, double *dw, double *gains, double *pbar, double *obsbar,
                                                       double *alpha, int S, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    return for_team_size(m, hipErrorInvalidValue, [&](auto M) {
        constexpr int M_ = decltype(M)::value;
        if (ofield)
            hipLaunchKernelGGL((sens_kernel<M_ + NMPC_SENS_OBS, KIND>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, wbar, dobs, rhs, dw, gains, pbar, obsbar, alpha, S, info, ws);
        else
            hipLaunchKernelGGL((sens_kernel<M_, KIND>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, wbar, dobs, rhs, dw, gains, pbar, obsbar, alpha, S, info, ws);
        return hipGetLastError();
    });
}

hipError_t launch_sens(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, double *dw, double *gains,
                       int gain_stages, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    return launch_sens_kind<SENS_PLAN>(P, m, B, w, lam_g, lam_x, dp, nullptr, nullptr, nullptr, dw, gains, nullptr, nullptr, nullptr, gain_stages, info, ws, st, ofield);
}

hipError_t launch_sens_adjoint(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *wbar, double *pbar,
                               double *obsbar, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    return launch_sens_kind<SENS_ADJOINT>(P, m, B, w, lam_g, lam_x, nullptr, wbar, nullptr, nullptr, nullptr, nullptr, pbar, obsbar, nullptr, obs_stages, info, ws, st, ofield);
}

hipError_t launch_sens_fwd(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                           const double *rhs, double *dw, double *alpha, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    return launch_sens_kind<SENS_UPDATE>(P, m, B, w, lam_g, lam_x, dp, nullptr, dobs, rhs, dw, nullptr, nullptr, nullptr, alpha, obs_stages, info, ws, st, ofield);
}

}  // namespace nmpc
