// nmpc_sens_adj.hip — adjoint plan sensitivities (include/nmpc.h, nmpc_sens_adjoint_batch): pbar = S_p' wbar and obsbar = S_o' wbar for a
// cotangent wbar of the plan.  The KKT matrix of the linearisation is symmetric, so the adjoint is the stage recursion of sens_kernel
// (nmpc_sens.hip) with a general affine column — -wbar on U_k and X_k, p_N = -wbar_{X_N}, where the forward-mode call has -2 Q dxs on X_k — and a
// forward pass from v_{X_0} = 0 that contracts v with 2 Q (the goal), with the obstacle blocks M_o of stages 1 .. N-1 (the field), and takes the
// measured state's part from the affine cost-to-go of stage 0.
//
// One wavefront per instance, in the layout of sens_kernel: lane j owns column j of [F | f] in the order [U_k; X_k | affine], assembled in LDS
// and eliminated in registers, [P_{k+1} | p_{k+1}] stays in LDS between stages, [G_k | g_k] of every stage goes to the pivot-row region [N][KTS]
// of the handle's workspace between the two passes.  The assembly of [B A]' P [B A] + W_k and the elimination are RESTATED from nmpc_sens.hip,
// not shared with it: with the body in one inlined function both kernels computed the parent's bits, but sens_kernel's generated code moved and
// its call ran 7 % slower, so that kernel stays as it is.  A change to the terms of W_k belongs in both files — and in
// nmpc_sens_fwd.hip and nmpc_sens_dual.hip, which state them again: a change to a term of W_k belongs in all four; the parity tables of the
// kernels (tests/sens_points.py) hold each against its own numpy reference.
// Sums over robots that share an obstacle and over stages that share an entry run in a fixed order inside the wavefront — no atomics, the same
// inputs give the same bits.
#include "nmpc_solve_common.h"

namespace nmpc {

// v of lane `lane` (a literal after unrolling), for every lane
__device__ __forceinline__ double lane_f64(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

constexpr int NMPC_SENS_OBS = 16;      // MS = team size + NMPC_SENS_OBS * (per-instance obstacle field), as sens_kernel's

// S: obs_stages of the call (1 or N; read only with obsbar)
template <int MS>
__global__ __launch_bounds__(64) void sens_adjoint_kernel(const KParams P, const double *__restrict__ w, const double *__restrict__ lam_g,
                                                          const double *__restrict__ lam_x, const double *__restrict__ wbar, double *__restrict__ pbar,
                                                          double *__restrict__ obsbar, int S, int32_t *__restrict__ info, double *__restrict__ ws)
{
    constexpr int M_ = MS % NMPC_SENS_OBS, OS = MS / NMPC_SENS_OBS;
    using G = G2<M_, 0>;
    constexpr int NX = G::NX, NU = G::NU, NZ = G::NZ, NP = G::NP;
    constexpr int LDF = NZ + 1, LDP = NX + 1, LDG = NX + 1;      // row strides of [F | f], [P | p] and, in the workspace, [G_k | g_k]
    static_assert(NZ + 1 <= 64, "one lane per column of the augmented stage matrix");
    static_assert(NU * LDG <= G::KTS, "[G_k | g_k] fits the stage's pivot-row slot of the workspace");
    static_assert(3 * NMPC_MAX_OBSTACLES <= 64, "one lane per entry of a stage's obstacle cotangent");
    __shared__ double F[NZ * LDF], Pb[NX * LDP], xk[NX], uk[NU], lx[NZ], lk[NX + NP + M_ * NMPC_MAX_OBSTACLES], cs[3 * M_], qx[NX], qu[NU], dx[NX], du[NU];
    const int j = threadIdx.x, N = P.N, K = P.K;
    const size_t b = blockIdx.x;
    const double *X = w + b * P.nvar, *U = X + (size_t)(N + 1) * NX;
    const double *lg = lam_g + b * P.ng, *lxX = lam_x + b * P.nvar, *lxU = lxX + (size_t)(N + 1) * NX;
    const double *wbX = wbar + b * P.nvar, *wbU = wbX + (size_t)(N + 1) * NX;
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

    // the linear term is -wbar, loaded stage by stage below; P_N = the bound terms of X_N, p_N = -wbar_{X_N}
    if (j <= NX)
        for (int r = 0; r < NX; r++) Pb[r * LDP + j] = j == NX ? -wbX[(size_t)N * NX + r] : 0.0;
    if (j < NX) Pb[j * LDP + j] = bterm(lxX[(size_t)N * NX + j], X[(size_t)N * NX + j], (j % 3 == 2) ? thub : P.xymax);
    lds_sync<64>();

#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
        // ---- the stage's point and multipliers: X_k, U_k, lam_x of both (X_0 carries none), lam_g of the stage block (defect, pair, obstacle rows)
        const double *lgk = lg + P.rows0 + (size_t)k * P.rowsk;
        if (j < NX) xk[j] = X[(size_t)k * NX + j];
        if (j < NU) uk[j] = U[(size_t)k * NU + j];
        if (j < NZ) lx[j] = isu ? lxU[(size_t)k * NU + j] : (k > 0 ? lxX[(size_t)k * NX + j - NU] : 0.0);
        if (j < NX) qx[j] = -wbX[(size_t)k * NX + j];
        if (j < NU) qu[j] = -wbU[(size_t)k * NU + j];
        for (int e = j; e < P.rowsk; e += 64) lk[e] = lgk[e];
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
#pragma unroll
            for (int i = 0; i < NU; i++) kt[(size_t)k * G::KTS + i * LDG + (j - NU)] = c[i];
#pragma unroll
            for (int r = 0; r < NX; r++) Pb[r * LDP + (j - NU)] = c[NU + r];
        }
        lds_sync<64>();
    }

    const int verdict = __ballot(bad) != 0 ? 2 : (indef ? 1 : 0);
    if (j == 0) info[b] = verdict;
    const int nob = 3 * K;      // entries of one stage of the obstacle cotangent: lane j < nob owns component j % 3 of obstacle j / 3
    if (verdict != 0) {      // no strict minimiser of the barrier problem, or no interior point: the instance's outputs are zeros
        if (pbar)
            for (int e = j; e < 2 * NX; e += 64) pbar[b * 2 * NX + e] = 0.0;
        if (obsbar)
            for (int e = j; e < S * nob; e += 64) obsbar[b * S * nob + e] = 0.0;
        return;
    }
    if (!pbar && !obsbar) return;
    // pbar_x0: the multiplier of the adjoint QP's initial block, minus the affine part p_0 of the stage-0 cost-to-go (<pbar, dp> = <wbar, S_p dp>)
    if (pbar && j < NX) pbar[b * 2 * NX + j] = -Pb[j * LDP + NX];
    // ---- forward pass from v_{X_0} = 0: v_{U_k} = G_k v_{X_k} + g_k, v_{X_{k+1}} = A_k v_{X_k} + B_k v_{U_k}.  Nothing of v is stored: the pass keeps
    //      sum_k 2 Q v_{X_k} (pbar_xs) and, at stages 1 .. N-1, -M_o' v: v_{X_k} against the obstacle blocks of the stage
    __syncthreads();      // the rows of [G_k | g_k] were written by other lanes
    double xsum = 0.0, osum = 0.0;
    if (j < NX) dx[j] = 0.0;
    lds_sync<64>();
#pragma unroll 1
    for (int k = 0; k < N; k++) {
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
        if (j < NU) {
            const double *g = kt + (size_t)k * G::KTS + j * LDG;
            double u = g[NX];
            for (int c = 0; c < NX; c++) u += g[c] * dx[c];
            du[j] = u;
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
    if (pbar && j < NX) pbar[b * 2 * NX + NX + j] = xsum;
    if (obsbar && S != N && j < nob) obsbar[b * nob + j] = osum;
}

template <int M_> static hipError_t launch_sens_adjoint_m(const KParams &P, int B, const double *w, const double *lam_g, const double *lam_x, const double *wbar,
                                                          double *pbar, double *obsbar, int S, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    if (ofield)
        hipLaunchKernelGGL((sens_adjoint_kernel<M_ + NMPC_SENS_OBS>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, wbar, pbar, obsbar, S, info, ws);
    else
        hipLaunchKernelGGL((sens_adjoint_kernel<M_>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, wbar, pbar, obsbar, S, info, ws);
    return hipGetLastError();
}

hipError_t launch_sens_adjoint(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *wbar, double *pbar,
                               double *obsbar, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    return for_team_size(m, hipErrorInvalidValue,
                         [&](auto M) { return launch_sens_adjoint_m<decltype(M)::value>(P, B, w, lam_g, lam_x, wbar, pbar, obsbar, obs_stages, info, ws, st, ofield); });
}

}  // namespace nmpc
