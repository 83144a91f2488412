// nmpc_ipm.h — the controller of the interior-point iteration, written once for the four solve kernels: solve_kernel
// (nmpc_kernels.hip), solve_lds_kernel (nmpc_solve_lds.hip), solve_col_kernel (nmpc_solve_col.hip) and lidar_solve_kernel (nmpc_lidar.hip).
//
// Plain scalar functions on wave-uniform values: no memory access, no thread index, no template parameters, no side effects beyond their
// arguments.  The state they steer stays in each kernel as scalars or as the small structs of scalars below.  What differs between the
// kernels stays visible at their call sites: where a rejected sweep resumes, what a cold retry does to mu and the phase, the uni() wrappers
// of the LIDAR kernel.  The CPU oracles (oracle/) restate the same rules independently and do not include this file.
//
// Compiles under hipcc (device code) and under a plain C++17 host compiler (tests/test_ipm_control_host.py).
#pragma once
#include <math.h>

#include "../../include/nmpc_constants.h"

#ifdef __HIPCC__
#define NMPC_IPM_FN __device__ __forceinline__
#else
#define NMPC_IPM_FN inline
#endif

namespace nmpc {
namespace ipm {

// ---- optimality error (IPOPT eq. 5) from the reduced residuals: e_d dual, e_c defects, e_h slack rows, lsum / zsum the 1-norms of the
// equality multipliers and the duals, szmax the largest complementarity product; n_rows equality multipliers plus inequality rows, n_ineq1 inequality
// rows, at least 1 (the caller forms and guards both)
struct OptErr {
    double s_d, s_c, E0;
};
NMPC_IPM_FN OptErr opt_error(double e_d, double e_c, double e_h, double lsum, double zsum, double szmax, double n_rows, double n_ineq1)
{
    const double smax = 100.0;
    OptErr r;
    r.s_d = fmax(smax, (lsum + zsum) / n_rows) / smax;
    r.s_c = fmax(smax, zsum / n_ineq1) / smax;
    r.E0 = fmax(fmax(e_d / r.s_d, e_c), fmax(e_h, szmax / r.s_c));
    return r;
}

// ---- monotone barrier update (IPOPT eq. 7): mu falls while the error of its barrier problem is within 10 mu; ed_sd = e_d / s_d
NMPC_IPM_FN double barrier_update(double mu, double tol, double ed_sd, double e_c, double e_h, double szmax, double szmin, double s_c)
{
    const double mu_min = tol / 10.0;
    for (;;) {
        const double cm = fmax(fabs(szmax - mu), fabs(szmin - mu));
        const double Emu = fmax(fmax(ed_sd, e_c), fmax(e_h, cm / s_c));
        if (mu > mu_min && Emu <= 10.0 * mu) mu = fmax(mu_min, fmin(0.2 * mu, pow(mu, 1.5)));
        else break;
    }
    return mu;
}
NMPC_IPM_FN double frac_to_boundary(double mu) { return fmax(0.99, 1.0 - mu); }      // tau of IPOPT eq. 15

// ---- inertia-shift schedule (IPOPT alg. IC).  First trial: no shift, except right after an iteration that needed one (a quarter of it).
NMPC_IPM_FN double shift_first(bool need_shift, double delta_last) { return need_shift ? fmax(1e-20, 0.25 * delta_last) : 0.0; }
// after a rejected pivot; the caller gives up once shift_exhausted()
NMPC_IPM_FN double shift_next(double delta, double delta_last)
{
    if (delta == 0.0) return (delta_last == 0.0) ? 1e-4 : fmax(1e-20, delta_last / 3.0);
    return delta * ((delta_last == 0.0) ? 100.0 : NMPC_SHIFT_ESCALATION);
}
NMPC_IPM_FN bool shift_exhausted(double delta) { return delta > 1e20; }
// after the accepted sweep (ntry rejected trials before it)
NMPC_IPM_FN void shift_accept(double delta, int ntry, double &delta_last, bool &need_shift)
{
    if (delta > 0.0) delta_last = delta;
    need_shift = delta > 0.0 && (ntry > 0 || delta > 1e-6);
}

// ---- penalty parameter of the l1 merit function, updated while the point is infeasible (th0 > 0, the caller's test): Nocedal-Wright
// (18.36), rho = 0.1, capped by the multiplier norm it cannot exceed in exact arithmetic.  The penalty may relax again (by half): one bad
// step must not cripple the rest of the solve.
NMPC_IPM_FN double penalty_update(double nu_pen, double dphi, double th0, double mult_max)
{
    const double nut = fmin(dphi / ((1.0 - 0.1) * th0), mult_max / (1.0 - 0.1));
    nu_pen = fmax(1.0, 0.5 * nu_pen);
    if (nu_pen < nut) nu_pen = nut + 1.0;
    return nu_pen;
}

// ---- non-monotone (Grippo-type) merit reference: the max of the current and the last three merit values of this barrier problem (mu, nu)
struct MeritRef {
    double h0 = 0.0, h1 = 0.0, h2 = 0.0, mu = -1.0, nu = -1.0;
    int count = 0;
    NMPC_IPM_FN void reset() { count = 0; }      // a (re)start of the barrier iteration, the watchdog
    NMPC_IPM_FN double reference(double mu_, double nu_, double m0)
    {
        if (mu != mu_ || nu != nu_) { count = 0; mu = mu_; nu = nu_; }
        double mref = m0;
        if (count > 0) mref = fmax(mref, h0);
        if (count > 1) mref = fmax(mref, h1);
        if (count > 2) mref = fmax(mref, h2);
        h2 = h1; h1 = h0; h0 = m0; if (count < 3) count++;
        return mref;
    }
};
// Armijo acceptance of the trial merit value at step length alpha; Dm the directional derivative of the merit function
NMPC_IPM_FN bool armijo(double m_trial, double mref, double alpha, double Dm, double phi0) { return m_trial <= mref + 1e-4 * alpha * Dm + 1e-13 * fabs(phi0); }

// ---- watchdog of the line search (include/nmpc_constants.h; the LIDAR kernel only): n_short counts the successive steps the backtracking shortened
NMPC_IPM_FN bool watchdog_fires(int n_short, double a_p) { return n_short >= NMPC_WATCHDOG_TRIGGER && a_p >= NMPC_WATCHDOG_MIN_AP; }
NMPC_IPM_FN int watchdog_count(int n_short, bool took, double alpha, double a_p) { return (!took && alpha < a_p) ? n_short + 1 : 0; }

// ---- stall and restart ladder: five successive steps below 1e-10 restart the barrier iteration from the current point, at most three
// times; then, on a NaN error, on a failed factorisation, or NMPC_COLD_RETRY_ITERS iterations into an attempt the solve restarts from the cold
// start, at most NMPC_COLD_RETRIES times; then it ends as stalled.
struct Ladder {
    int n_tiny = 0, n_restart = 0;      // successive tiny steps; barrier restarts of this attempt
    int n_cold = 0, it_base = 0;        // cold retries done; iteration at which the current attempt started
};
NMPC_IPM_FN void count_step(Ladder &l, double alpha) { l.n_tiny = (alpha < 1e-10) ? l.n_tiny + 1 : 0; }
NMPC_IPM_FN bool cold_retry_left(const Ladder &l) { return l.n_cold < NMPC_COLD_RETRIES; }
NMPC_IPM_FN bool cold_retry_due(const Ladder &l, int iter) { return l.n_cold < NMPC_COLD_RETRIES && iter - l.it_base >= NMPC_COLD_RETRY_ITERS; }
// bookkeeping of a cold retry; what it does to mu and the phase is the caller's (n_cold tells the first retry from the second)
NMPC_IPM_FN void cold_retry_begin(Ladder &l, int iter) { l.n_cold++; l.it_base = iter; l.n_tiny = 0; l.n_restart = 0; }
// after an accepted step: stalled() -> restarts_used_up() ? (cold_retry_left() ? cold retry : NMPC_STATUS_STALLED) : barrier restart, counted by
// barrier_restart_begin(), with mu = restart_mu()
NMPC_IPM_FN bool stalled(const Ladder &l) { return l.n_tiny >= 5; }
NMPC_IPM_FN bool restarts_used_up(const Ladder &l) { return l.n_restart >= 3; }
NMPC_IPM_FN void barrier_restart_begin(Ladder &l) { l.n_restart++; l.n_tiny = 0; }
NMPC_IPM_FN double restart_mu(double mu, double mu_init) { return fmax(mu, mu_init); }

}  // namespace ipm
}  // namespace nmpc
