// nmpc_sens_multi.hip — nmpc_sens_update_batch_multi (include/nmpc.h): the forward plan update of nmpc_sens_update_batch for D directions
// (dp, dobs, rhs)_d at the same primal-dual point (w, lam_g, lam_x) of every instance, in one launch of plan_dirs_kernel<MS>.  The matrix part
// of the stage recursion — [B A]' P [B A] + W_k, its n_u pivots, G_k, P_k — depends on the point only and is done once per stage; what repeats
// per direction is the affine column, its elimination against the pivots, and the forward pass.
//
// One wavefront per instance.  The lane map of the backward recursion, NZ = n_u + n_x, DC = 64 - NZ (59 for one robot .. 14 for ten;
// NMPC_QUERY_SENS_DIRS_PER_PASS):
//   lanes 0 .. NZ-1    column j of the stage matrix in the order [U_k; X_k], as in sens_kernel (nmpc_sens.hip);
//   lanes NZ .. 63     the affine column of one direction each: lane NZ + l carries direction g0 + l of the group g0, g0 + DC, .. being worked on.
// LDS holds [F | f_0 .. f_{DC-1}] at row stride 64 and the cost-to-go [P | p_0 .. p_{D-1}] at row stride n_x + NMPC_SENS_MAX_DIRS (ten robots:
// 25.0 + 22.0 KB), sized for D = NMPC_SENS_MAX_DIRS whatever D the call has.  A lane writes its own column only.  The first group is eliminated
// together with the matrix columns.  After pivot step i lane i is not touched again, so when D > DC the further groups load their affine
// columns into lanes NZ .. 63 and replay the same unrolled elimination and back-substitution against the registers of the matrix lanes, which are
// held (every update of a lane < NZ is masked off): the multipliers a later group reads by readlane are the very registers the first group
// read, and a direction's bits do not depend on its group, its lane or on D.
// [G_k] goes to the pivot-row region [N][KTS] of the handle's workspace as in sens_kernel; that slot has no room for D columns g_k, so g_k of
// direction d goes to the dU_k entries of that direction's dw, which the forward pass reads back and overwrites with dU_k = G_k dX_k + g_k —
// which is why dw is not optional here.
// The forward pass gives lane d direction d (D <= 64 = NMPC_SENS_MAX_DIRS): dX and dU of all directions stand in the LDS of F, entry-major
// ([n_x + n_u][64], the lane's own column, no bank conflict), every entry's sum runs in the order of sens_kernel, alpha is a plain minimum over
// the lane's items; what does not depend on the direction (sin, cos, the obstacle normals and slacks of the stage) is computed once per stage by
// the whole wave.  Global reads and writes of dw go through a (direction, entry) loop of the whole wave, so they are contiguous per direction.
//
// The stage recursion is restated here, not shared with nmpc_sens.hip through a function: the comment at the top of that file records what a
// function boundary costs in registers.  A term of W_k therefore lives in three places: sens_kernel (nmpc_sens.hip), plan_dirs_kernel (here),
// and, as a matrix-vector product, nmpc_sens_dual.hip — a change to one belongs in all three; tests/test_gpu_sens_multi.py holds this kernel
// against the numpy reference of the single-direction call (tests/sens_update_ref.py) per direction.
// Sums run in a fixed order — the terms of c at one entry: goal, rhs, then the obstacles in index order — no atomics: the same inputs give the
// same bits, in whatever slot a direction stands.
#include "nmpc_solve_common.h"

namespace nmpc {

// v of lane `lane` (a literal after unrolling), for every lane
__device__ __forceinline__ double dirs_lane_f64(double v, int lane)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// dp [B][D][2 nx], dobs [B][D][S][K][3], rhs [B][D][nvar] (each nullptr for zero), dw [B][D][nvar], alpha [B][D] or nullptr, info [B]; the host
// has checked 1 <= D <= NMPC_SENS_MAX_DIRS and S in {1, N}
template <int MS>
__global__ __launch_bounds__(64) void plan_dirs_kernel(const KParams P, const double *__restrict__ w, const double *__restrict__ lam_g, const double *__restrict__ lam_x,
                                                       const double *__restrict__ dp, const double *__restrict__ dobs, const double *__restrict__ rhs,
                                                       double *__restrict__ dw, double *__restrict__ alpha, int D, int S, int32_t *__restrict__ info, double *__restrict__ ws)
{
    constexpr int M_ = MS % NMPC_SENS_OBS, OS = MS / NMPC_SENS_OBS;
    using G = G2<M_, 0>;
    constexpr int NX = G::NX, NU = G::NU, NZ = G::NZ, NP = G::NP;
    constexpr int DC = 64 - NZ;                                          // affine columns per pass of the recursion
    constexpr int LDF = 64, LDP = NX + NMPC_SENS_MAX_DIRS, LDG = NX + 1;      // row strides of [F | f ..], [P | p ..] and, in the workspace, [G_k]
    constexpr int OGS = 5;                                               // doubles per (robot, obstacle) of the stage's obstacle geometry
    static_assert(DC >= 1 && NMPC_SENS_MAX_DIRS <= 64, "one lane per affine column; one lane per direction in the forward pass");
    static_assert(NU * LDG <= G::KTS, "[G_k] fits the stage's pivot-row slot of the workspace");
    static_assert(NP <= 64, "pair rows of a stage");
    __shared__ double F[NZ * LDF], Pb[NX * LDP], qb[NZ * DC], og[OGS * M_ * NMPC_MAX_OBSTACLES], xk[NX], uk[NU], lx[NZ], lk[NX + NP + M_ * NMPC_MAX_OBSTACLES], cs[3 * M_];
    const int j = threadIdx.x, N = P.N, K = P.K;
    const size_t b = blockIdx.x, nvar = (size_t)P.nvar;
    const double *X = w + b * nvar, *U = X + (size_t)(N + 1) * NX;
    const double *lg = lam_g + b * P.ng, *lxX = lam_x + b * nvar, *lxU = lxX + (size_t)(N + 1) * NX;
    const int nob = 3 * K;      // entries of one stage of dobs
    const size_t offU = (size_t)(N + 1) * NX;      // dU inside one direction's dw (and rhs)
    double *kt = ws + b * P.stride2 + P.oKT;       // [N][KTS], of which [NU][LDG] per stage are used here
    const ObsField<OS> OB(P, b);
    const int npairs = P.pairs ? NP : 0;
    const double T = P.T;
    // the variable of a matrix lane's column: control (rob, comp: 0 v, 1 omega) or state (rob, comp: 0 x, 1 y, 2 theta)
    const bool isu = j < NU, isx = j >= NU && j < NZ;
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

    // P_N = the bound terms of X_N; p_N of direction d = -rhs_{X_N}
    for (int e = j; e < NX * LDP; e += 64) Pb[e] = 0.0;
    lds_sync<64>();
    if (rhs)
        for (int t = j; t < D * NX; t += 64) {
            const int d = t / NX, r = t - d * NX;
            Pb[r * LDP + NX + d] = -rhs[(b * D + d) * nvar + (size_t)N * NX + r];
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
        for (int e = j; e < P.rowsk; e += 64) lk[e] = lgk[e];
        lds_sync<64>();
        if (j < M_) {
            double s, c;
            sincos(xk[3 * j + 2], &s, &c);
            cs[3 * j] = c; cs[3 * j + 1] = s; cs[3 * j + 2] = T * uk[2 * j];
        }
        // what the obstacle terms of c share between the directions, per (robot i, obstacle o): l, rr, n, Sigma with the slack rounded as in
        // the assembly below (s <= 0 there is verdict 2)
        if (dobs && k > 0)
            for (int e = j; e < M_ * K; e += 64) {
                const int i = e / K, o = e - i * K;
                const double l = lk[NX + npairs + e];
                const double ex = xk[3 * i] - OB(k, o, 0), ey = xk[3 * i + 1] - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey);
                og[OGS * e] = l; og[OGS * e + 1] = rr; og[OGS * e + 2] = ex / rr; og[OGS * e + 3] = ey / rr;
                og[OGS * e + 4] = -l > 0.0 ? -l / (rr - P.robdim - OB(k, o, 2) - P.margin) : 0.0;
            }
        lds_sync<64>();
        if (j < NZ) {
            // ---- [B A]' P [B A]: this lane's column of [B A] has the entries (r0, c0), (r1, c1), (r2, c2) —
            //      v_i: T cos, T sin on (x_i, y_i); omega_i: T on theta_i; x_i, y_i: 1; theta_i: 1 and -T v sin, T v cos on (x_i, y_i)
            const double c_ = cs[3 * rob], s_ = cs[3 * rob + 1], tv = cs[3 * rob + 2];
            int r0 = 0, r1 = 0, r2 = 0;
            double c0 = 1.0, c1 = 0.0, c2 = 0.0;
            if (isu) {
                if (comp == 0) { r0 = 3 * rob; c0 = T * c_; r1 = 3 * rob + 1; c1 = T * s_; }
                else { r0 = 3 * rob + 2; c0 = T; }
            } else {
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
            } else {
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
            }
        }
        lds_sync<64>();
        if (indef) continue;      // a pivot <= 0 further down the horizon: only the slacks of the remaining stages are still looked at (info 2)
        // ---- the groups of DC directions.  The first is eliminated with the matrix columns; the later ones replay the elimination against the
        //      registers of the lanes < NZ, which stay as the first group left them
        double c[NZ];
#pragma unroll 1
        for (int g0 = 0; g0 < D; g0 += DC) {
            const int nd = D - g0 < DC ? D - g0 : DC;
            // ---- the linear term c of the stage for the group's directions: entry e of X_k — the goal, then rhs, then (M_o dobs) of the robot's
            //      obstacle rows in index order (include/nmpc.h); stage 0 carries no obstacle term — and -rhs on U_k
            for (int t = j; t < nd * NX; t += 64) {
                const int dl = t / NX, e = t - dl * NX;
                const size_t bd = b * D + g0 + dl;
                double q = dp ? -2.0 * P.q[e % 3] * dp[bd * 2 * NX + NX + e] : 0.0;
                if (rhs) q -= rhs[bd * nvar + (size_t)k * NX + e];
                if (dobs && k > 0 && e % 3 < 2) {
                    const int i = e / 3, oc = e % 3;
                    const double *d = dobs + (bd * S + (S == N ? k : 0)) * nob;
                    for (int o = 0; o < K; o++) {
                        const double *gq = &og[OGS * (i * K + o)];
                        const double l = gq[0], rr = gq[1], n0 = gq[2], n1 = gq[3], sg = gq[4], nc = oc ? n1 : n0;
                        const double d0 = d[3 * o], d1 = d[3 * o + 1], ndd = n0 * d0 + n1 * d1;
                        q -= l * ((oc ? d1 : d0) - nc * ndd) / rr + sg * nc * ndd + sg * nc * d[3 * o + 2];
                    }
                }
                qb[(NU + e) * DC + dl] = q;
            }
            for (int t = j; t < nd * NU; t += 64) {
                const int dl = t / NU, e = t - dl * NU;
                qb[e * DC + dl] = rhs ? -rhs[(b * D + g0 + dl) * nvar + offU + (size_t)k * NU + e] : 0.0;
            }
            lds_sync<64>();
            const int dl = j - NZ, d = g0 + dl;
            const bool aff = j >= NZ && dl < nd;
            if (aff) {
                // [B A]' p of the direction: the column of [B A | e] is e itself, so the state rows start as p_{k+1}; the rows as above; + c
                for (int r = 0; r < NX; r++) F[(NU + r) * LDF + j] = Pb[r * LDP + NX + d];
                for (int i = 0; i < M_; i++) {
                    const double a0 = F[(NU + 3 * i) * LDF + j], a1 = F[(NU + 3 * i + 1) * LDF + j], a2 = F[(NU + 3 * i + 2) * LDF + j];
                    const double ci = cs[3 * i], si = cs[3 * i + 1], tvi = cs[3 * i + 2];
                    F[(2 * i) * LDF + j] = T * (ci * a0 + si * a1);
                    F[(2 * i + 1) * LDF + j] = T * a2;
                    F[(NU + 3 * i + 2) * LDF + j] = a2 + tvi * (ci * a1 - si * a0);
                }
                for (int e = 0; e < NZ; e++) F[e * LDF + j] += qb[e * DC + dl];
            }
            lds_sync<64>();
            // ---- the lane takes its column into registers and eliminates the n_u pivots there: the multiplier of row r is entry r of the pivot's
            //      column, read from the pivot's lane (fully unrolled: every register index and lane number is a literal).  An affine lane without
            //      a direction carries whatever its column of F holds; nothing reads it
            const bool act = g0 == 0 || j >= NZ;
#pragma unroll
            for (int r = 0; r < NZ; r++) c[r] = act ? F[r * LDF + j] : c[r];
#pragma unroll
            for (int i = 0; i < NU; i++) {
                const double dv = dirs_lane_f64(c[i], i);
                if (!(dv > 0.0)) indef = true;
                const bool upd = act && j > i;
                const double rd = 1.0 / dv, pj = c[i];
#pragma unroll
                for (int r = i + 1; r < NZ; r++) {
                    const double m = dirs_lane_f64(c[r], i) * rd;      // lane i itself is not updated in its own step
                    c[r] = upd ? c[r] - m * pj : c[r];
                }
            }
            if (indef) break;
            // ---- [G_k | g_k ..] = -F_uu^-1 [F_ux | f_u ..] by back-substitution in the state and affine columns (entry (i, l) of the factor:
            //      register i of lane l), then out; [P_k | p_k ..] for the next stage
#pragma unroll
            for (int i = NU - 1; i >= 0; i--) {
                double acc = c[i];
#pragma unroll
                for (int l = i + 1; l < NU; l++) acc += dirs_lane_f64(c[i], l) * c[l];
                const double gi = -acc / dirs_lane_f64(c[i], i);
                c[i] = (isu || !act) ? c[i] : gi;
            }
            if (g0 == 0 && isx) {
#pragma unroll
                for (int i = 0; i < NU; i++) kt[(size_t)k * G::KTS + i * LDG + (j - NU)] = c[i];
#pragma unroll
                for (int r = 0; r < NX; r++) Pb[r * LDP + (j - NU)] = c[NU + r];
            }
            if (aff) {
                double *gU = dw + (b * D + d) * nvar + offU + (size_t)k * NU;      // g_k of the direction: the forward pass turns it into dU_k
#pragma unroll
                for (int i = 0; i < NU; i++) gU[i] = c[i];
#pragma unroll
                for (int r = 0; r < NX; r++) Pb[r * LDP + NX + d] = c[NU + r];
            }
            lds_sync<64>();
        }
    }

    const int verdict = __ballot(bad) != 0 ? 2 : (indef ? 1 : 0);
    if (j == 0) info[b] = verdict;
    if (verdict != 0) {      // no strict minimiser of the barrier problem, or no interior point: every direction's outputs are zeros, and no step at all
        for (size_t e = j; e < (size_t)D * nvar; e += 64) dw[b * D * nvar + e] = 0.0;
        if (alpha && j < D) alpha[b * D + j] = 0.0;
        return;
    }
    // ---- forward pass, lane d = direction d, from dX_0 = dx0: dU_k = G_k dX_k + g_k, dX_{k+1} = A_k dX_k + B_k dU_k, and the alpha items of the
    //      stage the walk stands on: the smallest s / (-ds) over the items with s > 0 and ds < 0
    __syncthreads();      // the rows of [G_k] and the g_k were written by other lanes
    double *dxs = F, *dus = F + NX * 64;      // [NX][64], [NU][64]: entry-major, column = direction
    double amin = 1.0;
    auto item = [&](double s, double ds) { if (s > 0.0 && ds < 0.0) amin = fmin(amin, s / -ds); };
    // both sides of the bound -ub <= v <= ub along dv: upper s = ub - v, ds = -dv; lower s = v + ub, ds = dv
    auto bound = [&](double v, double dv, double ub) { if (ub < INFINITY) { item(ub - v, -dv); item(v + ub, dv); } };
    for (int t = j; t < D * NX; t += 64) {
        const int d = t / NX, e = t - d * NX;
        dxs[e * 64 + d] = dp ? dp[(b * D + d) * 2 * NX + e] : 0.0;
    }
    const bool dir = j < D;
    const double *dob = (dobs && dir) ? dobs + (b * D + j) * (size_t)S * nob : nullptr;
#pragma unroll 1
    for (int k = 0; k <= N; k++) {
        // ---- what the directions share at stage k: X_k, U_k, sin and cos of the headings, the obstacle normals and slacks; dX_k out, g_k in
        if (j < NX) xk[j] = X[(size_t)k * NX + j];
        if (k < N && j < NU) uk[j] = U[(size_t)k * NU + j];
        lds_sync<64>();
        if (k < N && j < M_) {
            double s, c;
            sincos(xk[3 * j + 2], &s, &c);
            cs[3 * j] = c; cs[3 * j + 1] = s; cs[3 * j + 2] = uk[2 * j];
        }
        if (alpha && k > 0 && k < N)
            for (int e = j; e < M_ * K; e += 64) {
                const int i = e / K, o = e - i * K;
                const double ex = xk[3 * i] - OB(k, o, 0), ey = xk[3 * i + 1] - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey);
                og[OGS * e] = ex / rr; og[OGS * e + 1] = ey / rr; og[OGS * e + 2] = rr - P.robdim - OB(k, o, 2) - P.margin;
            }
        for (int t = j; t < D * NX; t += 64) {
            const int d = t / NX, e = t - d * NX;
            dw[(b * D + d) * nvar + (size_t)k * NX + e] = dxs[e * 64 + d];
        }
        if (k < N)
            for (int t = j; t < D * NU; t += 64) {
                const int d = t / NU, e = t - d * NU;
                dus[e * 64 + d] = dw[(b * D + d) * nvar + offU + (size_t)k * NU + e];
            }
        lds_sync<64>();
        if (dir) {
            if (alpha && k > 0) {
                // the bounds of X_k, then (stages 1 .. N-1) the pair rows and the obstacle rows (robot i, obstacle o)
#pragma unroll 1
                for (int e = 0; e < NX; e++) bound(xk[e], dxs[e * 64 + j], (e % 3 == 2) ? thub : P.xymax);
                if (k < N) {
#pragma unroll 1
                    for (int q = 0; q < npairs; q++) {
                        int i = 0, a = 0;
                        pair_of<M_>(q, i, a);
                        const double ex = xk[3 * i] - xk[3 * a], ey = xk[3 * i + 1] - xk[3 * a + 1];
                        item(ex * ex + ey * ey - P.dmin2, 2.0 * (ex * (dxs[(3 * i) * 64 + j] - dxs[(3 * a) * 64 + j]) + ey * (dxs[(3 * i + 1) * 64 + j] - dxs[(3 * a + 1) * 64 + j])));
                    }
                    const double *d = dob ? dob + (S == N ? k : 0) * nob : nullptr;
#pragma unroll 1
                    for (int i = 0; i < M_; i++)
                        for (int o = 0; o < K; o++) {
                            const double *gq = &og[OGS * (i * K + o)];
                            const double d0 = d ? d[3 * o] : 0.0, d1 = d ? d[3 * o + 1] : 0.0, d2 = d ? d[3 * o + 2] : 0.0;
                            item(gq[2], gq[0] * (dxs[(3 * i) * 64 + j] - d0) + gq[1] * (dxs[(3 * i + 1) * 64 + j] - d1) - d2);
                        }
                }
            }
            if (k < N) {
#pragma unroll 1
                for (int e = 0; e < NU; e++) {
                    const double *g = kt + (size_t)k * G::KTS + e * LDG;
                    double u = dus[e * 64 + j];
                    for (int c = 0; c < NX; c++) u += g[c] * dxs[c * 64 + j];
                    dus[e * 64 + j] = u;
                    if (alpha) bound(uk[e], u, (e & 1) ? P.wmax : P.vmax);
                }
                // the robots one by one, in place: (x, y) take the old heading entry, then the heading moves
#pragma unroll 1
                for (int r = 0; r < M_; r++) {
                    const double c = cs[3 * r], s = cs[3 * r + 1], v = cs[3 * r + 2];
                    const double dv = dus[(2 * r) * 64 + j], dom = dus[(2 * r + 1) * 64 + j], dth = dxs[(3 * r + 2) * 64 + j];
                    dxs[(3 * r) * 64 + j] = dxs[(3 * r) * 64 + j] + T * (c * dv - v * s * dth);
                    dxs[(3 * r + 1) * 64 + j] = dxs[(3 * r + 1) * 64 + j] + T * (s * dv + v * c * dth);
                    dxs[(3 * r + 2) * 64 + j] = dth + T * dom;
                }
            }
        }
        lds_sync<64>();
        if (k < N)
            for (int t = j; t < D * NU; t += 64) {
                const int d = t / NU, e = t - d * NU;
                dw[(b * D + d) * nvar + offU + (size_t)k * NU + e] = dus[e * 64 + d];
            }
    }
    if (alpha && dir) alpha[b * D + j] = amin;
}

// one launch: the kernel of the team size, with or without the per-instance obstacle field
hipError_t launch_plan_dirs(const KParams &P, int m, int B, int D, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, double *dw, double *alpha, int obs_stages, int32_t *info, double *ws, hipStream_t st, bool ofield)
{
    if (D < 1 || D > NMPC_SENS_MAX_DIRS || !dw) return hipErrorInvalidValue;
    return for_team_size(m, hipErrorInvalidValue, [&](auto M) {
        constexpr int M_ = decltype(M)::value;
        if (ofield)
            hipLaunchKernelGGL((plan_dirs_kernel<M_ + NMPC_SENS_OBS>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, D, obs_stages, info, ws);
        else
            hipLaunchKernelGGL((plan_dirs_kernel<M_>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, D, obs_stages, info, ws);
        return hipGetLastError();
    });
}

int plan_dirs_per_pass(int m) { return m >= 1 && m <= NMPC_MAX_ROBOTS ? 64 - 5 * m : 0; }

}  // namespace nmpc
