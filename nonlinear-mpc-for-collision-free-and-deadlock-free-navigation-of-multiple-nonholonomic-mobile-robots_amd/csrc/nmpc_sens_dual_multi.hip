// nmpc_sens_dual_multi.hip — the multiplier updates of nmpc_sens_update_batch_multi_duals (include/nmpc.h): for the D directions whose dw
// plan_dirs_kernel<MS> (nmpc_sens_multi.hip) has written on the same stream, (dlam_g, dlam_x, dlam_p)_d complete the solution of the linearised
// barrier KKT system at fixed complementarity products, and alpha_dual_d says how much of them keeps every multiplier's sign.  The arithmetic is
// that of sens_dual_kernel<MS> (nmpc_sens_dual.hip): one backward walk dnu_{N-1} = -r_XN, dnu_{k-1} = A_k' dnu_k - r_Xk with the X rows of
// r_k = W_k [dU_k; dX_k] + c_k formed as a matrix-vector product, no elimination and no workspace.  A term of W_k therefore lives in four places —
// nmpc_sens.hip, nmpc_sens_multi.hip, nmpc_sens_dual.hip and this file; a change to one belongs in all four.  tests/test_gpu_sens_dual_multi.py
// holds this kernel against the numpy reference of the single-direction call (tests/sens_dual_ref.py) per direction.
//
// One wavefront per instance; lane d carries direction d (D <= 64 = NMPC_SENS_MAX_DIRS), lanes >= D take part in the shared work and in the
// cooperative loads and stores only.  Per stage the whole wave forms once what does not depend on the direction: cos, sin, T v and the two
// curvature terms of every robot (cs), beta of every variable of the stage (bt), per pair row (e_x, e_y, l, Sigma) (pg) and per (robot, obstacle)
// (l, rr, n, Sigma) (og, the pattern of plan_dirs_kernel).  dU_k and dX_k of all directions stand in LDS entry-major (dz [n_u + n_x][64]: a lane
// reads its own column, lane l on banks 2 l, 2 l + 1 of its 32-lane half: no conflict; the shared stage terms are read at one address by every
// lane: a broadcast), and so do the goal and rhs part of c_k (qt [n_x][64]) and the stage's dobs (ob [3 K][64], field instantiations only).
// Global reads of dw, dp, rhs and dobs go through a (direction, entry) loop of the whole wave, contiguous per direction.  dnu stays in the
// lane's registers, the entry loops unrolled over the compile-time n_x.
//
// Stores.  dlam_x,j = beta_j dw_j is elementwise, so the loop that loads dw stores it, contiguous per direction (the lane forms the same product
// again for its alpha_dual item and for r).  The rows of dlam_g go through a transposed tile: once the lane has used its column of qt, it writes
// up to n_x row values there — first dnu_{k-1}, which belongs to the rows of stage k - 1 (the initial block at k = 0), then the pair and obstacle
// rows of stage k in chunks of n_x — and the whole wave stores each chunk by a (direction, row) loop, n_x contiguous doubles per direction.
// alpha_dual is the lane's own running minimum: no wave reduction, no atomics.  dlam_p: the x0 part is the tile of dnu_init stored a second time
// (bit for bit dlam_g[:n_x]); the xs part is 2 Q (sum_k dX_k - N dxs), one (direction, entry) per lane after the walk, the sum taken over dw in
// the order of the walk, k = N-1 down to 0.
// A direction's bits depend on the point and the direction only: every lane runs the same instructions on its own column, and no value crosses
// lanes.
//
// Term order: the expressions of sens_dual_kernel — c_k: goal, rhs, then the obstacles in index order; r: 2 Q, the bound, the curvature, the
// pairs in robot order, then the obstacles in index order.  The three sums of two products that DESIGN.md section 5 names as the places where the
// compiler's fma contraction may differ between the kernels are left plain here, as in sens_dual_kernel, so the outputs agree with
// nmpc_sens_update_batch_duals to rounding, not bit for bit.
//
// As built (gfx950; tests/test_sens_dual_multi_host.py prints them), one .. ten robots: registers 126 / 146 / 153 / 163 / 167 / 175 / 175 / 185 /
// 189 / 197 without the field and 137 / 153 / 159 / 167 / 173 / 181 / 187 / 195 / 201 / 209 with it, no scratch in any; static LDS 4 704 / 9 376 /
// 14 144 / 18 896 / 23 760 / 28 592 / 33 520 / 38 432 / 43 456 / 48 448 bytes without the field and 12 288 more (ob) with it.  Ten robots with
// the field decide the layout: 25 600 (dz) + 15 360 (qt) + 12 288 (ob) + 7 488 of shared stage terms = 60 736 bytes, under the 64 KB a launch
// gets without opting in.  The per-instance bases of the D-slot arrays are formed once and indexed in 32 bits, and the robots of a stage are
// fenced from one another in the scheduler (sched_barrier): without either the compiler kept every robot's LDS reads in flight at once (510
// registers for ten robots) and reserved a private segment on some instantiations.
#include "nmpc_solve_common.h"

namespace nmpc {

// dp [B][D][2 nx], dobs [B][D][S][K][3], rhs [B][D][nvar] (each nullptr for zero), dw [B][D][nvar] and info [B] as plan_dirs_kernel<MS> left them;
// dlam_g [B][D][ng], dlam_x [B][D][nvar], dlam_p [B][D][2 nx], alpha_dual [B][D], each nullptr or written; the host has checked
// 1 <= D <= NMPC_SENS_MAX_DIRS and S in {1, N}
template <int MS>
__global__ __launch_bounds__(64) void dual_dirs_kernel(const KParams P, const double *__restrict__ w, const double *__restrict__ lam_g,
                                                       const double *__restrict__ lam_x, const double *__restrict__ dp, const double *__restrict__ dobs,
                                                       const double *__restrict__ rhs, const double *__restrict__ dw, int D, int S,
                                                       const int32_t *__restrict__ info, double *__restrict__ dlam_g, double *__restrict__ dlam_x,
                                                       double *__restrict__ dlam_p, double *__restrict__ alpha_dual)
{
    constexpr int M_ = MS % NMPC_SENS_OBS, OS = MS / NMPC_SENS_OBS;
    using G = G2<M_, 0>;
    constexpr int NX = G::NX, NU = G::NU, NZ = G::NZ, NP = G::NP;
    constexpr int CSS = 5, PGS = 4, OGS = 5;      // doubles per robot of cs, per pair row of pg, per (robot, obstacle) of og
    static_assert(NZ <= 64 && NP <= 64 && NMPC_SENS_MAX_DIRS <= 64, "one lane per entry, per pair row and per direction");
    __shared__ double dz[NZ * 64], qt[NX * 64], ob[OS ? 3 * NMPC_MAX_OBSTACLES * 64 : 1];
    __shared__ double xk[NX], uk[NU], lx[NZ], bt[NZ], lk[NX + NP + M_ * NMPC_MAX_OBSTACLES], cs[CSS * M_], pg[PGS * (NP > 0 ? NP : 1)], og[OGS * M_ * NMPC_MAX_OBSTACLES];
    const int j = threadIdx.x, N = P.N, K = P.K;
    const size_t b = blockIdx.x, bD = b * (size_t)D;
    const int nvar = P.nvar, ng = P.ng;
    const int offU = (N + 1) * NX;      // dU inside one direction's dw, and the U part inside lam_x and dlam_x
    const int nob = 3 * K;      // entries of one stage of dobs
    const bool hasd = OS != 0 && dobs != nullptr, hasr = rhs != nullptr, hasp = dp != nullptr;
    // the instance's D slots of every per-direction array: from here on an index is (slot d) * (the array's stride) + the entry, in 32 bits
    dw += bD * nvar;
    if (hasp) dp += bD * 2 * NX;
    if (hasr) rhs += bD * nvar;
    if (hasd) dobs += bD * S * nob;
    if (dlam_g) dlam_g += bD * ng;
    if (dlam_x) dlam_x += bD * nvar;
    if (dlam_p) dlam_p += bD * 2 * NX;
    if (alpha_dual) alpha_dual += bD;
    if (info[b] != 0) {      // verdict 1 or 2: no step at all, in any direction
        if (dlam_g)
            for (int e = j; e < D * ng; e += 64) dlam_g[e] = 0.0;
        if (dlam_x)
            for (int e = j; e < D * nvar; e += 64) dlam_x[e] = 0.0;
        if (dlam_p)
            for (int e = j; e < D * 2 * NX; e += 64) dlam_p[e] = 0.0;
        if (alpha_dual && j < D) alpha_dual[j] = 0.0;
        return;
    }
    const double *X = w + b * nvar, *U = X + offU;
    const double *lg = lam_g + b * ng, *lxX = lam_x + b * nvar, *lxU = lxX + offU;
    const ObsField<OS> OB(P, b);
    const int npairs = P.pairs ? NP : 0, nrow = npairs + M_ * K;      // the inequality rows of a stage
    const double T = P.T;
    const bool dir = j < D;
    // the variable of lane j's entry of [U_k; X_k], for the shared bound terms
    const bool isu = j < NU;
    const int comp = isu ? j % 2 : (j < NZ ? (j - NU) % 3 : 0);
    // a variable -ub <= v <= ub with multiplier l: max(l, 0) / (ub - v) + max(-l, 0) / (v + ub); the verdict is 0, so every such slack is positive
    auto bterm = [&](double l, double v, double ub) -> double {
        double t = 0.0;
        if (ub < INFINITY && (l > 0.0 || l < 0.0)) t = fabs(l) / (l > 0.0 ? ub - v : v + ub);
        return t;
    };
    // an inequality row g >= lb with multiplier l and slack s = g - lb: Sigma = max(-l, 0) / s
    auto sigma = [&](double l, double s) -> double { return -l > 0.0 ? -l / s : 0.0; };
    const double thub = P.thb ? P.thmax : INFINITY;
    // alpha_dual of the lane's direction: the smallest z / (-dz) over the items with z > 0 and dz < 0
    double amin = 1.0;
    auto item = [&](double z, double dzv) { if (z > 0.0 && dzv < 0.0) amin = fmin(amin, z / -dzv); };
    // the bound of entry e of the stage vector moves its multiplier l by t dv: exactly 0.0 without a term; z = |l|, dz = sign(l) t dv
    auto bound = [&](int e, double dv) -> double {
        const double l = lx[e], t = bt[e];
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
    // entry e of a direction's dw -> dz, and beta_e dw_e -> dlam_x, for `n` entries per direction starting at `src` inside dw and at row `z0` of dz
    auto load_dw = [&](int n, int src, int z0) {
        for (int t = j; t < D * n; t += 64) {
            const int d = t / n, e = t - d * n;
            const double v = dw[d * nvar + src + e], tb = bt[z0 + e];
            dz[(z0 + e) * 64 + d] = v;
            if (dlam_x) dlam_x[d * nvar + src + e] = tb > 0.0 ? tb * v : 0.0;
        }
    };
    // the first n rows of the tile, all directions -> rows row0 .. of dlam_g (and, with `init`, the x0 part of dlam_p)
    auto store_rows = [&](int n, int row0, bool init) {
        lds_sync<64>();
        for (int t = j; t < D * n; t += 64) {
            const int d = t / n, v = t - d * n;
            const double val = qt[v * 64 + d];
            if (dlam_g) dlam_g[d * ng + row0 + v] = val;
            if (init && dlam_p) dlam_p[d * 2 * NX + v] = val;
        }
        lds_sync<64>();
    };
    double nu[NX];      // dnu of the stage above, of the lane's direction: registers (every index below is a literal)

    // ---- X_N: r = the bound terms of X_N times dX_N - rhs; dnu_{N-1} = -r
    if (j < NX) {
        const int e = N * NX + j;
        lx[NU + j] = lxX[e];
        bt[NU + j] = bterm(lxX[e], X[e], (j % 3 == 2) ? thub : P.xymax);
    }
    lds_sync<64>();
    load_dw(NX, N * NX, NU);
    if (hasr)
        for (int t = j; t < D * NX; t += 64) {
            const int d = t / NX, e = t - d * NX;
            qt[e * 64 + d] = rhs[d * nvar + N * NX + e];
        }
    if (dlam_g)      // the pad rows
        for (int t = j; t < D * (P.rows0 - NX); t += 64) {
            const int d = t / (P.rows0 - NX), e = t - d * (P.rows0 - NX);
            dlam_g[d * ng + NX + e] = 0.0;
        }
    lds_sync<64>();
    static_for<0, NX>([&](auto E) {
        constexpr int e = decltype(E)::value;
        nu[e] = 0.0;
        if (dir) {
            const double d = bound(NU + e, dz[(NU + e) * 64 + j]);
            nu[e] = -(hasr ? d - qt[e * 64 + j] : d);
            qt[e * 64 + j] = nu[e];
        }
    });
    store_rows(NX, P.rows0 + (N - 1) * P.rowsk, false);

#pragma unroll 1
    for (int k = N - 1; k >= 0; k--) {
        // ---- the stage's point and multipliers: X_k, U_k, lam_x of both (X_0 carries none), lam_g of the stage block
        const int rowk = P.rows0 + k * P.rowsk;      // the stage's block inside lam_g and dlam_g
        const double *lgk = lg + rowk;
        if (j < NX) xk[j] = X[k * NX + j];
        if (j < NU) uk[j] = U[k * NU + j];
        if (j < NZ) lx[j] = isu ? lxU[k * NU + j] : (k > 0 ? lxX[k * NX + j - NU] : 0.0);
        for (int e = j; e < P.rowsk; e += 64) lk[e] = lgk[e];
        lds_sync<64>();
        // ---- what the directions share: per robot cos, sin, T v, the heading curvature d2 L / d theta^2 and the cross term d2 L / d theta d v;
        //      beta of every entry; per pair row (e_x, e_y, l, Sigma); per (robot, obstacle) (l, rr, n, Sigma)
        if (j < M_) {
            double s, c;
            sincos(xk[3 * j + 2], &s, &c);
            const double tv = T * uk[2 * j], l0 = lk[3 * j], l1 = lk[3 * j + 1];
            cs[CSS * j] = c; cs[CSS * j + 1] = s; cs[CSS * j + 2] = tv;
            cs[CSS * j + 3] = tv * (l0 * c + l1 * s);
            cs[CSS * j + 4] = T * (l0 * s - l1 * c);
        }
        if (j < NZ) bt[j] = isu ? bterm(lx[j], uk[j], comp ? P.wmax : P.vmax) : bterm(lx[j], xk[j - NU], comp == 2 ? thub : P.xymax);      // X_0: lx is 0.0, no term
        if (k > 0) {
            if (j < npairs) {
                int i = 0, a = 0;
                pair_of<M_>(j, i, a);
                const double l = lk[NX + j];
                const double ex = xk[3 * i] - xk[3 * a], ey = xk[3 * i + 1] - xk[3 * a + 1];
                pg[PGS * j] = ex; pg[PGS * j + 1] = ey; pg[PGS * j + 2] = l; pg[PGS * j + 3] = sigma(l, ex * ex + ey * ey - P.dmin2);
            }
            for (int e = j; e < M_ * K; e += 64) {
                const int i = e / K, o = e - i * K;
                const double l = lk[NX + npairs + e];
                const double ex = xk[3 * i] - OB(k, o, 0), ey = xk[3 * i + 1] - OB(k, o, 1), rr = sqrt(ex * ex + ey * ey);
                og[OGS * e] = l; og[OGS * e + 1] = rr; og[OGS * e + 2] = ex / rr; og[OGS * e + 3] = ey / rr;
                og[OGS * e + 4] = sigma(l, rr - P.robdim - OB(k, o, 2) - P.margin);
            }
        }
        lds_sync<64>();
        // ---- dX_k, dU_k of every direction in, their bound multipliers out; the goal and rhs part of c_k; the stage's dobs
        load_dw(NX, k * NX, NU);
        load_dw(NU, offU + k * NU, 0);
        for (int t = j; t < D * NX; t += 64) {
            const int d = t / NX, e = t - d * NX;
            double q = hasp ? -2.0 * P.q[e % 3] * dp[d * 2 * NX + NX + e] : 0.0;
            if (hasr) q -= rhs[d * nvar + k * NX + e];
            qt[e * 64 + d] = q;
        }
        if (hasd && k > 0)
            for (int t = j; t < D * nob; t += 64) {
                const int d = t / nob, c = t - d * nob;
                ob[c * 64 + d] = dobs[(d * S + (S == N ? k : 0)) * nob + c];
            }
        lds_sync<64>();
        // ---- lane d, direction d: the bounds of U_k, then robot by robot the X rows of r_k = W_k [dU_k; dX_k] + c_k and
        //      dnu_{k-1} = A_k' dnu_k - r_Xk (A_k = I, and its heading column carries -T v sin, T v cos on (x_i, y_i))
#pragma unroll 1
        for (int e = 0; e < (dir ? NU : 0); e++) bound(e, dz[e * 64 + j]);      // r_Uk - B_k' dnu_k = 0 holds by the choice of dU_k and defines nothing
        static_for<0, M_>([&](auto I) {
            constexpr int i = decltype(I)::value;
            if (dir) {
                const double c_ = cs[CSS * i], s_ = cs[CSS * i + 1], tv = cs[CSS * i + 2], hth = cs[CSS * i + 3], cross = cs[CSS * i + 4];
                const double dxi = dz[(NU + 3 * i) * 64 + j], dyi = dz[(NU + 3 * i + 1) * 64 + j], dth = dz[(NU + 3 * i + 2) * 64 + j];
                double r0 = 2.0 * P.q[0] * dxi + bound(NU + 3 * i, dxi);
                double r1 = 2.0 * P.q[1] * dyi + bound(NU + 3 * i + 1, dyi);
                double r2 = 2.0 * P.q[2] * dth + bound(NU + 3 * i + 2, dth);
                r2 += hth * dth + cross * dz[(2 * i) * 64 + j];
                double q0 = qt[(3 * i) * 64 + j], q1 = qt[(3 * i + 1) * 64 + j];
                const double q2 = qt[(3 * i + 2) * 64 + j];
                if (k > 0) {      // the pair and obstacle rows of stages 1 .. N-1 (those of stage 0 act on the pinned X_0: nothing)
#pragma unroll 1
                    for (int a = 0; a < (npairs ? M_ : 0); a++) {
                        if (a == i) continue;
                        const double *g = &pg[PGS * pidx_any<M_>(i, a)];      // the row holds e of the pair in index order
                        const double ex = i < a ? g[0] : -g[0], ey = i < a ? g[1] : -g[1], l = g[2];
                        const double sg = 4.0 * g[3];      // grad g = 2 (e, -e) on (robot i, robot a)
                        const double ddx = dxi - dz[(NU + 3 * a) * 64 + j], ddy = dyi - dz[(NU + 3 * a + 1) * 64 + j];
                        r0 += sg * ex * (ex * ddx + ey * ddy) + 2.0 * l * ddx;
                        r1 += sg * ey * (ex * ddx + ey * ddy) + 2.0 * l * ddy;
                    }
#pragma unroll 1
                    for (int o = 0; o < K; o++) {
                        const double *g = &og[OGS * (i * K + o)];
                        const double l = g[0], rr = g[1], n0 = g[2], n1 = g[3], sg = g[4];      // grad g = n; Hessian (I - n n') / r
                        const double ndw = n0 * dxi + n1 * dyi;
                        r0 += l * (dxi - n0 * ndw) / rr + sg * n0 * ndw;
                        r1 += l * (dyi - n1 * ndw) / rr + sg * n1 * ndw;
                        if (hasd) {      // (M_o dobs) of the robot's rows
                            const double d0 = ob[(3 * o) * 64 + j], d1 = ob[(3 * o + 1) * 64 + j], d2 = ob[(3 * o + 2) * 64 + j], ndd = n0 * d0 + n1 * d1;
                            q0 -= l * (d0 - n0 * ndd) / rr + sg * n0 * ndd + sg * n0 * d2;
                            q1 -= l * (d1 - n1 * ndd) / rr + sg * n1 * ndd + sg * n1 * d2;
                        }
                    }
                }
                const double a0 = nu[3 * i], a1 = nu[3 * i + 1], a2 = nu[3 * i + 2] + tv * (c_ * nu[3 * i + 1] - s_ * nu[3 * i]);
                nu[3 * i] = a0 - (r0 + q0);
                nu[3 * i + 1] = a1 - (r1 + q1);
                nu[3 * i + 2] = a2 - (r2 + q2);
            }
            __builtin_amdgcn_sched_barrier(0);      // one robot at a time: without it the scheduler hoists every robot's LDS reads to the top of the stage and spills
        });
        // ---- dnu_{k-1}: the defect rows of stage k - 1, or the initial block (and the x0 part of dlam_p)
        if (dir)
            static_for<0, NX>([&](auto E) { qt[decltype(E)::value * 64 + j] = nu[decltype(E)::value]; });
        store_rows(NX, k > 0 ? rowk - P.rowsk : 0, k == 0);
        // ---- the stage's inequality rows: Sigma_i ds_i on stages 1 .. N-1 with the ds of the update's alpha items, 0.0 on stage 0
        if (k > 0) {
#pragma unroll 1
            for (int v0 = 0; v0 < nrow; v0 += NX) {
                const int cnt = nrow - v0 < NX ? nrow - v0 : NX;
                if (dir) {
#pragma unroll 1
                    for (int v = 0; v < cnt; v++) {
                        const int rw = v0 + v;
                        double val;
                        if (rw < npairs) {
                            int i = 0, a = 0;
                            pair_of<M_>(rw, i, a);
                            const double *g = &pg[PGS * rw];
                            val = row(g[2], g[3], 2.0 * (g[0] * (dz[(NU + 3 * i) * 64 + j] - dz[(NU + 3 * a) * 64 + j]) +
                                                         g[1] * (dz[(NU + 3 * i + 1) * 64 + j] - dz[(NU + 3 * a + 1) * 64 + j])));
                        } else {
                            const int e = rw - npairs, i = e / K, o = e - i * K;
                            const double *g = &og[OGS * e];
                            const double d0 = hasd ? ob[(3 * o) * 64 + j] : 0.0, d1 = hasd ? ob[(3 * o + 1) * 64 + j] : 0.0, d2 = hasd ? ob[(3 * o + 2) * 64 + j] : 0.0;
                            val = row(g[0], g[4], g[2] * (dz[(NU + 3 * i) * 64 + j] - d0) + g[3] * (dz[(NU + 3 * i + 1) * 64 + j] - d1) - d2);
                        }
                        qt[v * 64 + j] = val;
                    }
                }
                store_rows(cnt, rowk + NX + v0, false);
            }
        } else if (dlam_g) {
            for (int t = j; t < D * nrow; t += 64) {
                const int d = t / nrow, e = t - d * nrow;
                dlam_g[d * ng + rowk + NX + e] = 0.0;
            }
        }
    }
    // ---- the xs part of dlam_p: 2 Q (sum_{k<N} dX_k - N dxs), the sum in the order of the walk
    if (dlam_p)
        for (int t = j; t < D * NX; t += 64) {
            const int d = t / NX, e = t - d * NX;
            const double *dX = dw + d * nvar + e;
            double sum = 0.0;
            for (int k = N - 1; k >= 0; k--) sum += dX[k * NX];
            const double dxs = hasp ? dp[d * 2 * NX + NX + e] : 0.0;
            dlam_p[d * 2 * NX + NX + e] = 2.0 * P.q[e % 3] * (sum - (double)N * dxs);
        }
    if (alpha_dual && dir) alpha_dual[j] = amin;
}

// one launch behind launch_plan_dirs on its stream: the kernel of the team size, with or without the per-instance obstacle field
hipError_t launch_dual_dirs(const KParams &P, int m, int B, int D, const double *w, const double *lam_g, const double *lam_x, const double *dp, const double *dobs,
                            const double *rhs, const double *dw, int obs_stages, const int32_t *info, double *dlam_g, double *dlam_x, double *dlam_p,
                            double *alpha_dual, hipStream_t st, bool ofield)
{
    if (D < 1 || D > NMPC_SENS_MAX_DIRS || !dw) return hipErrorInvalidValue;
    return for_team_size(m, hipErrorInvalidValue, [&](auto M) {
        constexpr int M_ = decltype(M)::value;
        if (ofield)
            hipLaunchKernelGGL((dual_dirs_kernel<M_ + NMPC_SENS_OBS>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, D, obs_stages, info,
                               dlam_g, dlam_x, dlam_p, alpha_dual);
        else
            hipLaunchKernelGGL((dual_dirs_kernel<M_>), dim3((unsigned)B), dim3(64), 0, st, P, w, lam_g, lam_x, dp, dobs, rhs, dw, D, obs_stages, info, dlam_g,
                               dlam_x, dlam_p, alpha_dual);
        return hipGetLastError();
    });
}

}  // namespace nmpc
