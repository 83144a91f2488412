// nmpc_sens_dual.hip — the multiplier updates that go with the forward plan update (include/nmpc.h, nmpc_sens_update_batch_duals): given the dw
// that sens_kernel<MS, SENS_UPDATE> (nmpc_sens.hip) has written, (dlam_g, dlam_x) complete the solution of the linearised barrier KKT system at fixed
// complementarity products, and alpha_dual says how much of them keeps every multiplier's sign.
//
// Nothing is eliminated here.  With r = W dw + c (W and c as in nmpc_sens.hip, SENS_UPDATE) stationarity in X_k reads r_Xk + dnu_{k-1} - A_k' dnu_k = 0
// for the multipliers dnu_k of the linearised defects X_{k+1} - (X_k + T f), so one backward walk gives them all: dnu_{N-1} = -r_XN,
// dnu_{k-1} = A_k' dnu_k - r_Xk, dnu_init = A_0' dnu_0 - r_X0.  The X rows of r_k = W_k [dU_k; dX_k] + c_k are formed as a matrix-vector product
// from the terms of W_k, never as a matrix (the U rows define nothing: r_Uk - B_k' dnu_k = 0 holds by the choice of dU_k): a term of W_k lives in two places, nmpc_sens.hip and this
// file, and a change to one belongs in both; the parity tables (tests/sens_points.py) hold each kernel against its own numpy reference.  The inequality rows get Sigma_i ds_i with the
// ds of the update's alpha items, the bounds beta_j dw_j.
//
// One wavefront per instance: lane j < NZ owns entry j of the stage vector [U_k; X_k], the pair rows of a stage go to lanes j < NP, its obstacle
// rows through a strided loop (ten robots among eight obstacles have 80).  dnu of the current stage, dX_k, dU_k and the stage's lam_g block live
// in LDS; no workspace.  The terms of c at one entry are added in sens_kernel's order, alpha_dual is one wave-wide minimum: no atomics, the
// same inputs give the same bits.
#include "nmpc_solve_common.h"

namespace nmpc {

// MS = team size + NMPC_SENS_OBS * (per-instance obstacle field), as sens_kernel's.  S: obs_stages of the call (1 or N; read only with dobs).  info [B] holds the verdicts sens_kernel<MS, SENS_UPDATE> wrote on the same stream.
template <int MS>
__global__ __launch_bounds__(64) void sens_dual_kernel(const KParams P, const double *__restrict__ w, const double *__restrict__ lam_g,
                                                       const double *__restrict__ lam_x, const double *__restrict__ dp, const double *__restrict__ dobs,
                                                       const double *__restrict__ rhs, const double *__restrict__ dw, int S,
                                                       const int32_t *__restrict__ info, double *__restrict__ dlam_g, double *__restrict__ dlam_x,
                                                       double *__restrict__ alpha_dual)
{
    constexpr int M_ = MS % NMPC_SENS_OBS, OS = MS / NMPC_SENS_OBS;
    using G = G2<M_, 0>;
    constexpr int NX = G::NX, NU = G::NU, NZ = G::NZ, NP = G::NP;
    static_assert(NZ <= 64, "one lane per entry of the stage vector");
    static_assert(NP <= 64, "one lane per pair row of a stage");
    __shared__ double xk[NX], uk[NU], lx[NZ], lk[NX + NP + M_ * NMPC_MAX_OBSTACLES], cs[3 * M_], qx[NX], dx[NX], du[NU], nu[NX], nn[NX];
    const int j = threadIdx.x, N = P.N, K = P.K;
    const size_t b = blockIdx.x;
    double *dg = dlam_g ? dlam_g + b * P.ng : nullptr;
    double *dlX = dlam_x ? dlam_x + b * P.nvar : nullptr, *dlU = dlam_x ? dlX + (size_t)(N + 1) * NX : nullptr;
    if (info[b] != 0) {      // verdict 1 or 2: no step at all
        if (dg)
            for (int e = j; e < P.ng; e += 64) dg[e] = 0.0;
        if (dlX)
            for (int e = j; e < P.nvar; e += 64) dlX[e] = 0.0;
        if (alpha_dual && j == 0) alpha_dual[b] = 0.0;
        return;
    }
    const double *X = w + b * P.nvar, *U = X + (size_t)(N + 1) * NX;
    const double *dX = dw + b * P.nvar, *dU = dX + (size_t)(N + 1) * NX;
    const double *lg = lam_g + b * P.ng, *lxX = lam_x + b * P.nvar, *lxU = lxX + (size_t)(N + 1) * NX;
    const double *rhX = rhs ? rhs + b * P.nvar : nullptr;      // the U part of rhs enters dw alone
    const int nob = 3 * K;      // entries of one stage of dobs
    const double *dob = dobs ? dobs + b * (size_t)S * nob : nullptr;
    const ObsField<OS> OB(P, b);
    const int npairs = P.pairs ? NP : 0;
    const double T = P.T;
    // the variable of this lane's entry: control (rob, comp: 0 v, 1 omega) or state (rob, comp: 0 x, 1 y, 2 theta)
    const bool isu = j < NU, isx = j >= NU && j < NZ;
    const int rob = isu ? j / 2 : (isx ? (j - NU) / 3 : 0), comp = isu ? j % 2 : (isx ? (j - NU) % 3 : 0);
    // a variable -ub <= v <= ub with multiplier l: max(l, 0) / (ub - v) + max(-l, 0) / (v + ub); the verdict is 0, so every such slack is positive
    auto bterm = [&](double l, double v, double ub) -> double {
        double t = 0.0;
        if (ub < INFINITY && (l > 0.0 || l < 0.0)) t = fabs(l) / (l > 0.0 ? ub - v : v + ub);
        return t;
    };
    // an inequality row g >= lb with multiplier l and slack s = g - lb: Sigma = max(-l, 0) / s
    auto sigma = [&](double l, double s) -> double { return -l > 0.0 ? -l / s : 0.0; };
    const double thub = P.thb ? P.thmax : INFINITY;
    // alpha_dual: the smallest z / (-dz) over the items with z > 0 and dz < 0, a lane's own minimum first
    double amin = 1.0;
    auto item = [&](double z, double dz) { if (z > 0.0 && dz < 0.0) amin = fmin(amin, z / -dz); };
    // a bound's multiplier l moves by t dv: dlam_x = t dv (exactly 0.0 without a term), z = |l|, dz = sign(l) t dv
    auto bound = [&](double l, double t, double dv) -> double {
        const double d = t > 0.0 ? t * dv : 0.0;
        item(fabs(l), l > 0.0 ? d : -d);
        return d;
    };
    // an inequality row's multiplier l <= 0 moves by sg ds (exactly 0.0 without a Sigma): z = -l, dz = -sg ds
    auto row = [&](double l, double sg, double ds) -> double {
        const double d = sg > 0.0 ? sg * ds : 0.0;
        item(-l, -d);
        return d;
    };

    // the goal's part of the linear term, -2 Q dxs on every X_k, k < N
    const double qgoal = (dp && j < NX) ? -2.0 * P.q[j % 3] * dp[b * 2 * NX + NX + j] : 0.0;
    // ---- X_N: r = the bound terms of X_N times dX_N - rhs; dnu_{N-1} = -r
    if (j < NX) {
        const size_t e = (size_t)N * NX + j;
        const double d = bound(lxX[e], bterm(lxX[e], X[e], (j % 3 == 2) ? thub : P.xymax), dX[e]);
        if (dlX) dlX[e] = d;
        nu[j] = -(rhX ? d - rhX[e] : d);
    }
    if (dg)
        for (int e = NX + j; e < P.rows0; e += 64) dg[e] = 0.0;      // the pad rows
    lds_sync<64>();

#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
        // ---- the stage's point, multipliers and step: X_k, U_k, lam_x of both (X_0 carries none), lam_g of the stage block, dX_k, dU_k
        const double *lgk = lg + P.rows0 + (size_t)k * P.rowsk;
        double *dgk = dg ? dg + P.rows0 + (size_t)k * P.rowsk : nullptr;
        if (j < NX) { xk[j] = X[(size_t)k * NX + j]; dx[j] = dX[(size_t)k * NX + j]; }
        if (j < NU) { uk[j] = U[(size_t)k * NU + j]; du[j] = dU[(size_t)k * NU + j]; }
        if (j < NZ) lx[j] = isu ? lxU[(size_t)k * NU + j] : (k > 0 ? lxX[(size_t)k * NX + j - NU] : 0.0);
        for (int e = j; e < P.rowsk; e += 64) lk[e] = lgk[e];
        if (dgk && j < NX) dgk[j] = nu[j];      // dnu_k, from the stage above
        // ---- the linear term c of the stage in sens_kernel's order: the goal, then rhs, then (M_o dobs) of the robot's obstacle rows in index order
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
                    const double sg = -l > 0.0 ? -l / (rr - P.robdim - OB(k, o, 2) - P.margin) : 0.0;
                    const double d0 = d[3 * o], d1 = d[3 * o + 1], nd = n0 * d0 + n1 * d1;
                    q -= l * ((oc ? d1 : d0) - nc * nd) / rr + sg * nc * nd + sg * nc * d[3 * o + 2];
                }
            }
            qx[j] = q;
        }
        lds_sync<64>();
        if (j < M_) {
            double s, c;
            sincos(xk[3 * j + 2], &s, &c);
            cs[3 * j] = c; cs[3 * j + 1] = s; cs[3 * j + 2] = T * uk[2 * j];
        }
        lds_sync<64>();
        // ---- entry j of the X rows of r_k = W_k [dU_k; dX_k] + c_k: 2 Q, the heading / speed curvature of the defects, the bound terms, the pair and
        //      obstacle blocks with their Sigma parts; the bound's own multiplier step on the way
        if (j < NZ) {
            const double c_ = cs[3 * rob], s_ = cs[3 * rob + 1], tv = cs[3 * rob + 2];
            const double l0 = lk[3 * rob], l1 = lk[3 * rob + 1];
            const double cross = T * (l0 * s_ - l1 * c_);      // d2 L / d theta_i d v_i
            if (isu) {
                // the rows of U_k take part with their bound alone: r_Uk - B_k' dnu_k = 0 holds by the choice of dU_k and defines nothing
                const double d = bound(lx[j], bterm(lx[j], uk[j], comp ? P.wmax : P.vmax), du[j]);
                if (dlU) dlU[(size_t)k * NU + j] = d;
            } else {
                const int e = j - NU;
                double d = 0.0;
                if (k > 0) d = bound(lx[j], bterm(lx[j], xk[e], comp == 2 ? thub : P.xymax), dx[e]);
                if (dlX) dlX[(size_t)k * NX + e] = d;      // X_0: 0.0
                double r = 2.0 * P.q[comp] * dx[e] + d;
                if (comp == 2) r += tv * (l0 * c_ + l1 * s_) * dx[e] + cross * du[2 * rob];
                if (comp < 2 && k > 0) {      // the pair and obstacle rows of stages 1 .. N-1 (those of stage 0 act on the pinned X_0: nothing)
                    const double xi = xk[3 * rob], yi = xk[3 * rob + 1], dxi = dx[3 * rob], dyi = dx[3 * rob + 1], dc = comp ? dyi : dxi;
                    for (int a = 0; a < (npairs ? M_ : 0); a++) {
                        if (a == rob) continue;
                        const double l = lk[NX + pidx_any<M_>(rob, a)];
                        const double ex = xi - xk[3 * a], ey = yi - xk[3 * a + 1], ed = comp ? ey : ex;
                        const double sg = 4.0 * sigma(l, ex * ex + ey * ey - P.dmin2);      // grad g = 2 (e, -e) on (robot i, robot a)
                        const double ddx = dxi - dx[3 * a], ddy = dyi - dx[3 * a + 1];
                        r += sg * ed * (ex * ddx + ey * ddy) + 2.0 * l * (comp ? ddy : ddx);
                    }
                    for (int o = 0; o < K; o++) {
                        const double l = lk[NX + npairs + rob * K + o];
                        const double ex = xi - OB(k, o, 0), ey = yi - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey), n0 = ex / rr, n1 = ey / rr, nd = comp ? n1 : n0;
                        const double sg = sigma(l, rr - P.robdim - OB(k, o, 2) - P.margin);      // grad g = n; Hessian (I - n n') / r
                        const double ndw = n0 * dxi + n1 * dyi;
                        r += l * (dc - nd * ndw) / rr + sg * nd * ndw;
                    }
                }
                // ---- dnu_{k-1} = A_k' dnu_k - r_Xk: A_k = I, and its heading column carries -T v sin, T v cos on (x_i, y_i)
                double an = nu[e];
                if (comp == 2) an += tv * (c_ * nu[3 * rob + 1] - s_ * nu[3 * rob]);
                nn[e] = an - (r + qx[e]);
            }
        }
        // ---- the stage's inequality rows: Sigma_i ds_i on stages 1 .. N-1 with the ds of the update's alpha items, 0.0 on stage 0
        if (k > 0) {
            if (j < npairs) {
                int i = 0, a = 0;
                pair_of<M_>(j, i, a);
                const double l = lk[NX + j];
                const double ex = xk[3 * i] - xk[3 * a], ey = xk[3 * i + 1] - xk[3 * a + 1];
                const double d = row(l, sigma(l, ex * ex + ey * ey - P.dmin2), 2.0 * (ex * (dx[3 * i] - dx[3 * a]) + ey * (dx[3 * i + 1] - dx[3 * a + 1])));
                if (dgk) dgk[NX + j] = d;
            }
            const double *d = dob ? dob + (S == N ? k : 0) * nob : nullptr;
            for (int e = j; e < M_ * K; e += 64) {
                const int i = e / K, o = e % K;
                const double l = lk[NX + npairs + e];
                const double ex = xk[3 * i] - OB(k, o, 0), ey = xk[3 * i + 1] - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey), n0 = ex / rr, n1 = ey / rr;
                const double d0 = d ? d[3 * o] : 0.0, d1 = d ? d[3 * o + 1] : 0.0, d2 = d ? d[3 * o + 2] : 0.0;
                const double v = row(l, sigma(l, rr - P.robdim - OB(k, o, 2) - P.margin), n0 * (dx[3 * i] - d0) + n1 * (dx[3 * i + 1] - d1) - d2);
                if (dgk) dgk[NX + npairs + e] = v;
            }
        } else if (dgk) {
            for (int e = NX + j; e < P.rowsk; e += 64) dgk[e] = 0.0;
        }
        lds_sync<64>();
        if (j < NX) nu[j] = nn[j];
        lds_sync<64>();
    }
    if (dg && j < NX) dg[j] = nu[j];      // the initial block: dnu_init
    if (alpha_dual) {
        const double a = wave_min(amin);
        if (j == 0) alpha_dual[b] = a;
    }
}

template <int M_> static hipError_t launch_sens_dual_m(const KParams &P, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp,
                                                       const double *dobs, const double *rhs, const double *dw, int S, const int32_t *info, double *dlam_g,
                                                       double *dlam_x, double *alpha_dual, hipStream_t st, bool ofield)
{
    if (ofield)
        hipLaunchKernelGGL((sens_dual_kernel<M_ + NMPC_SENS_OBS>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, S, info, dlam_g,
                           dlam_x, alpha_dual);
    else
        hipLaunchKernelGGL((sens_dual_kernel<M_>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, S, info, dlam_g, dlam_x, alpha_dual);
    return hipGetLastError();
}

hipError_t launch_sens_dual(const KParams &P, int m, int B, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, const double *dw, int obs_stages, const int32_t *info, double *dlam_g, double *dlam_x, double *alpha_dual,
                            hipStream_t st, bool ofield)
{
    return for_team_size(m, hipErrorInvalidValue, [&](auto M) {
        return launch_sens_dual_m<decltype(M)::value>(P, B, w, lam_g, lam_x, dp, dobs, rhs, dw, obs_stages, info, dlam_g, dlam_x, alpha_dual, st, ofield);
    });
}

}  // namespace nmpc
