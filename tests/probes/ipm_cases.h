// ipm_cases.h — one call of a controller rule of csrc/nmpc_ipm.h per table row, written once for the device (wave_probe.hip) and for the host
// compiler (ipm_cases_host.cpp), so that the two sides run the same text on the same inputs.  It defines no rule itself and holds no expected
// value.  Row: in[0] the rule, in[1..11] its arguments (and, for the rules with state, the state before the call); out[0..7] what the rule
// returned (and the state after it).  Unused slots are written as 0.
#pragma once
#include "nmpc_ipm.h"

namespace ipm_cases {

enum { IN = 12, OUT = 8 };
enum { OPT_ERROR = 0, BARRIER_UPDATE, FRAC_TO_BOUNDARY, SHIFT, SHIFT_ACCEPT, PENALTY_UPDATE, MERIT_REF, ARMIJO, WATCHDOG, LADDER, RESTART_MU };

NMPC_IPM_FN void apply(const double *in, double *out)
{
    using namespace nmpc::ipm;
    for (int k = 0; k < OUT; k++) out[k] = 0.0;
    const double *a = in + 1;
    switch ((int)in[0]) {
    case OPT_ERROR: { const OptErr r = opt_error(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); out[0] = r.s_d; out[1] = r.s_c; out[2] = r.E0; break; }
    case BARRIER_UPDATE: out[0] = barrier_update(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); break;
    case FRAC_TO_BOUNDARY: out[0] = frac_to_boundary(a[0]); break;
    case SHIFT:      // (need_shift, delta, delta_last)
        out[0] = shift_first(a[0] != 0.0, a[2]); out[1] = shift_next(a[1], a[2]); out[2] = shift_exhausted(a[1]) ? 1.0 : 0.0; break;
    case SHIFT_ACCEPT: {      // (delta, ntry, delta_last, need_shift)
        double dl = a[2]; bool ns = a[3] != 0.0;
        shift_accept(a[0], (int)a[1], dl, ns); out[0] = dl; out[1] = ns ? 1.0 : 0.0; break;
    }
    case PENALTY_UPDATE: out[0] = penalty_update(a[0], a[1], a[2], a[3]); break;
    case MERIT_REF: {      // state (h0, h1, h2, mu, nu, count), then (mu_, nu_, m0, reset before the call)
        MeritRef h; h.h0 = a[0]; h.h1 = a[1]; h.h2 = a[2]; h.mu = a[3]; h.nu = a[4]; h.count = (int)a[5];
        if (a[9] != 0.0) h.reset();
        out[0] = h.reference(a[6], a[7], a[8]);
        out[1] = h.h0; out[2] = h.h1; out[3] = h.h2; out[4] = h.mu; out[5] = h.nu; out[6] = (double)h.count; break;
    }
    case ARMIJO: out[0] = armijo(a[0], a[1], a[2], a[3], a[4]) ? 1.0 : 0.0; break;
    case WATCHDOG:      // (n_short, took, alpha, a_p)
        out[0] = watchdog_fires((int)a[0], a[3]) ? 1.0 : 0.0; out[1] = (double)watchdog_count((int)a[0], a[1] != 0.0, a[2], a[3]); break;
    case LADDER: {      // state (n_tiny, n_restart, n_cold, it_base), then (alpha, iter, action: 0 none, 1 barrier restart, 2 cold retry)
        Ladder l; l.n_tiny = (int)a[0]; l.n_restart = (int)a[1]; l.n_cold = (int)a[2]; l.it_base = (int)a[3];
        const int iter = (int)a[5], act = (int)a[6];
        count_step(l, a[4]);
        out[0] = stalled(l) ? 1.0 : 0.0; out[1] = restarts_used_up(l) ? 1.0 : 0.0; out[2] = cold_retry_left(l) ? 1.0 : 0.0; out[3] = cold_retry_due(l, iter) ? 1.0 : 0.0;
        if (act == 1) barrier_restart_begin(l);
        if (act == 2) cold_retry_begin(l, iter);
        out[4] = (double)l.n_tiny; out[5] = (double)l.n_restart; out[6] = (double)l.n_cold; out[7] = (double)l.it_base; break;
    }
    case RESTART_MU: out[0] = restart_mu(a[0], a[1]); break;
    default: break;
    }
}

}  // namespace ipm_cases
