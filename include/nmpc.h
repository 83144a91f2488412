/*
 * nmpc.h — C ABI of the MI355X batched NMPC solver (libnmpc_hip.so).
 *
 * Drop-in boundary for the per-timestep solve of the reference scripts
 *   AS = AllScripts/ of asalimil/Nonlinear-MPC-for-collision-free-and-deadlock-free-
 *        navigation-of-multiple-nonholonomic-mobile-robots
 *   C6 = AS/centralized_six_robots_implementation.py
 *
 * The reference has no FFI of its own: the boundary it exposes is the CasADi solver
 * object call plus shift():
 *     solver = nlpsol('solver','ipopt', nlp_prob, opts)          C6:345-346
 *     sol    = solver(x0=,p=,lbx=,ubx=,lbg=,ubg=)                C6:432
 *     t0, u0 = shift(T, t0, u)                                   C6:160-169,450
 * Each entry point below names the block it replaces.  All buffers are caller-owned
 * DEVICE pointers (fp64 / int32), row-major with the batch index leading.  No global
 * state (the library reads no environment variable; what is not a literal of a reference
 * script is an explicit nmpc_options_t); every call is ordered on the hipStream_t passed as `void *stream` (NULL = the
 * default stream).  Return value: 0 on success, negative NMPC_E_* on argument / HIP
 * errors.  Non-convergence is NOT an error (the reference never reads solver.stats());
 * it is reported per instance in `status`.
 *
 * Concurrency: a handle owns ONE device workspace that every solve on it uses, so one
 * handle must not be used from two streams or two host threads at the same time (the
 * reference's loop is single-threaded and blocking, C6:416-465); different handles are
 * independent.  The handle remembers the device it was created on; every call makes
 * that device current for its own duration, and all buffers and the stream passed to a
 * call must belong to it.
 */
#ifndef NMPC_H_
#define NMPC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMPC_MAX_ROBOTS 10
#define NMPC_MAX_OBSTACLES 8

/* per-instance solve status */
#define NMPC_STATUS_CONVERGED 0      /* scaled KKT error <= tol                                  */
#define NMPC_STATUS_MAX_ITER 1       /* iteration limit hit; last iterate returned               */
#define NMPC_STATUS_NUMERIC 2        /* inertia correction exhausted / non-finite step           */
#define NMPC_STATUS_INFEASIBLE_X0 3  /* a stage-0 pair/obstacle row is violated by the pinned x0 */
#define NMPC_STATUS_STALLED 4        /* the restarts of last resort are spent (barrier restarts, the cold start, the elastic phase — where
                                        IPOPT runs its restoration phase) and the iteration still stalls, or the elastic phase converged with
                                        an elastic variable open: a stationary point of the infeasibility; last iterate returned */

/* return codes */
#define NMPC_OK 0
#define NMPC_E_ARG (-1)
#define NMPC_E_UNSUPPORTED (-2)
#define NMPC_E_HIP (-3)
#define NMPC_E_NOMEM (-4)

/*
 * Every literal of one reference script (C6:197-205 T,N,m,dmin,v_max,omega_max;
 * C6:252-266 Q,R; C6:349-352 bounds; obstacle literals
 * AS/third_scenario_mpc_obstacle_avoidance.py:58,97-119,175-177).
 */
typedef struct nmpc_config {
    int32_t m;              /* robots: 1..10 (the reference scripts use 1..6, 8 and 10; 7 and 9 are instantiated since round 4); beyond -> NMPC_E_UNSUPPORTED */
    int32_t N;              /* horizon, 2..4096                                                 */
    int32_t n_obs;          /* static circular obstacles, 0..NMPC_MAX_OBSTACLES                 */
    int32_t pad_rows;       /* 1: initial g block carries M constant rows (C6:278); 0: it does not */
    double T;               /* sample time                                                      */
    double dmin;            /* pair rows bounded below by dmin^2 (C6:349)                       */
    double q[3];            /* Q diagonal per robot                                             */
    double r[2];            /* R diagonal per robot                                             */
    double v_max, w_max;    /* |v| <= v_max, |omega| <= w_max                                   */
    double xy_max;          /* |x|,|y| <= xy_max (10 in every script)                           */
    double th_max;          /* |theta| <= th_max; +inf = unbounded (multi-robot scripts)        */
    double rob_dim, margin; /* obstacle rows: sqrt(.) - rob_dim - obs_r >= margin               */
    double pad_value;       /* 3.5 (C6:278)                                                     */
    double obs[3 * NMPC_MAX_OBSTACLES]; /* (ox, oy, obs_r) per obstacle                         */
    /* solver options: the 'ipopt' dict of C6:345 plus IPOPT defaults that matter */
    double tol;             /* 1e-8 (acceptable_tol of C6:345 == IPOPT tol)                     */
    double mu_init;         /* 0.5: initial barrier parameter (IPOPT ships 0.1; 0.5 saves ~13% iterations) */
    int32_t max_iter;       /* reference: 2000                                                  */
    int32_t pair_rows;      /* 1: pairwise collision rows present (C6:288-306); 0: the multi-robot NLP WITHOUT them
                               (AS/mpc_online_casadi_tb3_multi_centralized.py:115-148: g has 3m(N+1) rows, no padding rows) */
} nmpc_config_t;

typedef struct nmpc_handle nmpc_handle_t;

/* sizes implied by a config */
int32_t nmpc_n_var(const nmpc_config_t *cfg); /* n_x (N+1) + n_u N                    (C6:339) */
int32_t nmpc_n_g(const nmpc_config_t *cfg);   /* rows of g in the reference's order   (C6:278,326-331) */
int32_t nmpc_n_p(const nmpc_config_t *cfg);   /* 2 n_x                                (C6:241) */

/* fills *cfg with the defaults above and the Q/R/bounds literals shared by all scripts */
void nmpc_config_default(nmpc_config_t *cfg, int32_t m, int32_t N);

/*
 * Replaces nlpsol('solver','ipopt',nlp_prob,opts) (C6:342-346): validates the config and
 * allocates a device workspace for up to max_batch instances.
 */
int32_t nmpc_create(const nmpc_config_t *cfg, int32_t max_batch, nmpc_handle_t **out);
int32_t nmpc_destroy(nmpc_handle_t *h);

/*
 * Creation options that are not literals of a reference script.  nmpc_create(cfg, B, out) is nmpc_create_opts(cfg, B, NULL, out).
 */
typedef struct nmpc_options {
    int32_t kernel;         /* 0: the library picks the solve kernel per batch size (default).  1 HBM-resident, 2 element-per-lane,
                               3 column-per-lane in its throughput shape (one wavefront per instance), 4 / 5 column-per-lane in its latency
                               shape with two / four wavefronts per instance (four: five and six robots, else two): that kernel for every
                               batch size it can run (tests, A/B measurements)                                                         */
    int32_t trace_instance; /* -DNMPC_PROFILE builds: instance whose per-iteration trace is recorded (include/nmpc_debug.h); -1 none */
} nmpc_options_t;
int32_t nmpc_create_opts(const nmpc_config_t *cfg, int32_t max_batch, const nmpc_options_t *opts, nmpc_handle_t **out);

/*
 * Facts about a handle.  Returns the value, or a negative NMPC_E_* code.
 *   NMPC_QUERY_KERNEL_FOR_BATCH  arg = B: the solve kernel nmpc_solve_batch launches for a batch of B: 1 / 2 / 3 as in nmpc_options_t, 4 = the
 *                                column kernel's latency shape (two OR four wavefronts per instance: 5 is a pin, never an answer)
 *   NMPC_QUERY_WORKSPACE_BYTES   device workspace held by the handle (same as nmpc_workspace_bytes)
 *   NMPC_QUERY_LDS_BYTES         arg = B: dynamic LDS per swarm instance of the kernel an UNORDERED call of B gets (0 for the HBM-resident kernel's fixed
 *                                carve-up; for the element-per-lane kernel the bytes of its throughput shape whatever B: its latency shapes take a little more)
 *   NMPC_QUERY_MAX_BATCH         the max_batch the handle was created for
 *   NMPC_QUERY_KERNEL_FOR_ORDERED_BATCH  arg = B: as NMPC_QUERY_KERNEL_FOR_BATCH for a call that carries a dispatch-order hint
 *                                (nmpc_solve_batch_ordered, nmpc_step_batch): the latency shape is kept for larger batches then
 *   NMPC_QUERY_SENS_DIRS_PER_PASS  how many directions of nmpc_sens_update_batch_multi the handle's kernel carries through one pass of its stage
 *                                recursion (64 - 5 m: the lanes of a wavefront the stage matrix leaves free); a call with more directions repeats
 *                                only the affine part of the recursion for every further group of that size
 */
#define NMPC_QUERY_KERNEL_FOR_BATCH 1
#define NMPC_QUERY_WORKSPACE_BYTES 2
#define NMPC_QUERY_LDS_BYTES 3
#define NMPC_QUERY_MAX_BATCH 4
#define NMPC_QUERY_KERNEL_FOR_ORDERED_BATCH 5
#define NMPC_QUERY_SENS_DIRS_PER_PASS 6
int64_t nmpc_query(const nmpc_handle_t *h, int32_t what, int64_t arg);

/* bytes of device workspace held by the handle */
int64_t nmpc_workspace_bytes(const nmpc_handle_t *h);

/*
 * Replaces sol = solver(x0=,p=,lbx=,ubx=,lbg=,ubg=) (C6:432) for B independent swarms.
 *   p      [B][2 n_x]   parameters [x0; xs]                       (C6:419)
 *   w0     [B][n_var]   initial guess [X_0..X_N; U_0..U_{N-1}]     (C6:423)
 *   w_out  [B][n_var]   sol['x']                                   (C6:436,440)
 *   obj    [B]          sol['f']           (may be NULL)
 *   status [B] iters[B] kkt[B]             (may be NULL)
 * Bounds are those of the config (the scripts never change them between calls).
 * Stream-ordered; a handle owns ONE workspace.  A launch lasts as long as its longest solve: to keep the device busy over a stream of batches use two
 * handles on two streams and alternate the launches (bench.py `two_streams`: six robots, B = 4096, 277 k -> 445 k solves/s).
 */
int32_t nmpc_solve_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *w0, double *w_out,
                         double *obj, int32_t *status, int32_t *iters, double *kkt, void *stream);

/*
 * nmpc_solve_batch with a dispatch-order hint: order [B] (device, int32) is a permutation of 0..B-1 and workgroup g solves
 * instance order[g]; results land at the instance's own index, exactly as without the hint.  The launch takes as long as
 * "start of the longest solve + its length", so a caller that can rank the instances by expected effort (in a receding-horizon
 * loop: by the iteration counts of the previous control period, rank correlation 0.6-0.7) puts the long ones first.
 * order == NULL is nmpc_solve_batch.  No reference counterpart (the reference solves one instance per call, C6:432).
 * A hint that is not a permutation (an entry out of range or repeated) is detected on the device before the solve and
 * ignored for that call (the batch is then solved in index order): a bad hint costs time, never results or memory safety.
 */
int32_t nmpc_solve_batch_ordered(nmpc_handle_t *h, int32_t B, const double *p, const double *w0, double *w_out, double *obj,
                                 int32_t *status, int32_t *iters, double *kkt, const int32_t *order, void *stream);

/*
 * Evaluates the NLP functions in the reference's layout at w: f (C6:314) and
 * g [B][n_g] (C6:278,318-331).  Backs sol['f'] / sol['g'] of the host wrapper.
 */
int32_t nmpc_eval_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *w, double *f, double *g,
                        void *stream);

/*
 * Replaces shift() and the warm-start row shuffle (C6:160-169,450,460-465):
 *   U rows: drop first, duplicate last;  X rows: [X_1..X_N; X_{N-1}].
 * x0_next [B][n_x] may be NULL; when given it is written as the plant step
 *   x0 + T f(x0, u_0) of AS/casadi_test.py:17-26 (x0 read from p_in[:, :n_x]).
 * w_in and w_next must not alias.
 */
int32_t nmpc_shift_batch(nmpc_handle_t *h, int32_t B, const double *p_in, const double *w_in, double *w_next,
                         double *x0_next, void *stream);

/*
 * One control period of the receding-horizon loop for B swarms, entirely on the device and on one stream (C6:416-465 with the plant of
 * AS/casadi_test.py:17-26, the stack SURVEY.md 3(C) describes): nmpc_solve_batch_ordered, then nmpc_shift_batch, then the dispatch order
 * of the next period — no host round trip in between.
 *   p      [B][2 n_x]  in: [x0; xs]; out: x0 replaced by the plant step x0 + T f(x0, u_0) of the solution (xs untouched: the caller
 *                      changes goals between calls)                                                       (casadi_test.py:17-26,170)
 *   w      [B][n_var]  in: the guess; out: the next guess, the shifted solution [X_1..X_N; X_{N-1}], [U_1..U_{N-1}; U_{N-1}]   (C6:450,465)
 *   w_sol  [B][n_var]  out: sol['x'] of this period (its row U_0 is the control to apply, C6:444); must not alias w
 *   obj, status, iters, kkt: as nmpc_solve_batch (may be NULL)
 *   order  [B] int32   in: dispatch order of this period (a permutation of 0..B-1; anything else is detected and ignored);
 *                      out: the instances sorted by this period's iteration counts, longest first — the hint for the next call.
 *                      May be NULL (index order, no hint produced).  A caller's first call passes the identity.
 * Failed solves: an instance that ends with NMPC_STATUS_NUMERIC (2: the iterate may be non-finite) or NMPC_STATUS_INFEASIBLE_X0 (3) keeps its
 * x0 and its guess — its rows of p and w are NOT overwritten (w_sol holds what the solve returned); statuses 1 and 4 return a finite last
 * iterate and are shifted like a converged one, as the scripts do with any IPOPT return.
 */
int32_t nmpc_step_batch(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, double *obj, int32_t *status, int32_t *iters,
                        double *kkt, int32_t *order, void *stream);

/*
 * Obstacles as per-instance solve parameters, static or moving.  The three calls below are nmpc_solve_batch_ordered, nmpc_step_batch and
 * nmpc_eval_batch with the obstacle field of every instance instead of the handle's:
 *   obs [B][S][K][3] fp64 device, (ox, oy, r) per obstacle; K = cfg.n_obs of the handle; S = obs_stages, 1 or N.
 *   Stage k's obstacle rows (k = 0..N-1, evaluated at X_k) use entry k when S == N and entry 0 when S == 1, i.e. entry k is the obstacle at
 *   the time of X_k (a moving obstacle: its predicted path; a growing radius: prediction uncertainty).  The handle's cfg.obs values are not
 *   read by these calls; a handle for K parametric obstacles is a config with n_obs = K.
 * The row layout, n_g, the bounds (margin on every obstacle row) and the status codes are those of the plain calls; NMPC_STATUS_INFEASIBLE_X0
 * uses entry 0 of the instance's own field.  The field is read by the instance, never by the workgroup: with a dispatch-order hint, workgroup
 * g solves instance order[g] with obs[order[g]].  Given the same field as the config, the results are bit-identical to the plain calls.
 * Returns NMPC_E_ARG when cfg.n_obs == 0, obs == NULL with B > 0, or obs_stages is neither 1 nor N; otherwise the errors of the plain call.
 * Kernels: only the column-per-lane kernel has the per-instance field, in every shape (throughput; latency, two or four wavefronts per
 * instance); where the plain call would run the element-per-lane kernel, these run the column kernel's throughput shape.  Handles that run on
 * kernel 1 or 2 (horizons too long for the column kernel's LDS, or nmpc_options_t.kernel = 1 / 2) get NMPC_E_UNSUPPORTED from the two solve
 * calls; nmpc_eval_batch_obs works on every handle.
 */
int32_t nmpc_solve_batch_obs(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w0, double *w_out,
                             double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order, void *stream);   /* order may be NULL */
int32_t nmpc_step_batch_obs(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *obs, int32_t obs_stages, double *obj,
                            int32_t *status, int32_t *iters, double *kkt, int32_t *order, void *stream);
int32_t nmpc_eval_batch_obs(nmpc_handle_t *h, int32_t B, const double *p, const double *w, const double *obs, int32_t obs_stages, double *f, double *g,
                            void *stream);

/*
 * The solver's own multipliers: sol['lam_g'], sol['lam_x'], sol['lam_p'] of the CasADi call (C6:432), and a KKT certificate of any
 * (w, lam_g, lam_x) for a whole batch on the device.
 *
 * Convention (CasADi's): L = f + lam_g' g + lam_x' w + lam_p' p with grad_w L = 0 and grad_p L = 0 at a solution; a multiplier is <= 0 on an
 * active lower bound and >= 0 on an active upper bound.  The layouts are those of g, w and p everywhere else in this header (the row order
 * of nmpc_eval_batch).
 *   lam_g [B][n_g]   defect rows of stage k (g = X_{k+1} - F(X_k, U_k)): the solver's multiplier of that defect, with the sign of that g;
 *                    pair and obstacle rows of stages 1..N-1: minus the solver's dual z >= 0 (the rows are bounded below, so the value is <= 0);
 *                    pad rows: 0;
 *                    pair and obstacle rows of stage 0: 0 BY DEFINITION — they act on the pinned X_0, the solver gives them no slack, and the
 *                    constraint qualification fails there;
 *                    initial block X_0 - x0: from stationarity in X_0, -(2 Q (X_0 - xs) + (d c_0 / d X_0)' lam_g[c_0]) with c_0 the defect of
 *                    stage 0 — it absorbs whatever the stage-0 rows would carry.
 *   lam_x [B][n_var] controls: (dual of the upper bound) - (dual of the lower bound); bounded components of X_1..X_N: the same; X_0: 0;
 *                    headings when th_max = +inf: 0.
 *   lam_p [B][n_p]   the x0 part equals lam_g[:n_x] (bit for bit); the xs part is 2 Q sum_{k<N} (X_k - xs).  Both follow from grad_p L = 0, so
 *                    d f* / d p = -lam_p: the sensitivity of the optimal cost to the measured state and to the goal.
 * By status: 0 (including a solve that converged in the elastic phase with its elastic variables closed): the multipliers of the returned
 * point, for which the solve's own optimality test held; 1 / 4: those of the last iterate; 2: whatever the iterate holds, possibly non-finite;
 * 3 (the return before the iteration): all three rows are zero.
 *
 * nmpc_solve_batch_duals / nmpc_step_batch_duals are nmpc_solve_batch_ordered / nmpc_step_batch (obs == NULL and obs_stages == 0: the
 * handle's own obstacle field) or nmpc_solve_batch_obs / nmpc_step_batch_obs (otherwise, by their rules) that also write the multipliers;
 * order may be NULL.  Each member of *duals is a device pointer or NULL (not written); duals == NULL, or all three members NULL, is exactly
 * the call without multipliers, and w_out, obj, status, iters, kkt never depend on them.  The step call returns the multipliers of this
 * period's w_sol.  The multipliers are written by the column-per-lane kernel (every shape): where the plain call would run the
 * element-per-lane kernel these run the column kernel's throughput shape, and handles that run on kernel 1 or 2 get NMPC_E_UNSUPPORTED from
 * both calls (as from the *_obs calls).
 *
 * nmpc_kkt_batch evaluates, for given w [B][n_var], lam_g [B][n_g], lam_x [B][n_var] (any: a solve's output or a caller's own),
 *   grad_lag [B][n_var] = grad f + J' lam_g + lam_x   (written when not NULL; the stage-0 rows enter with the multipliers given) and
 *   res [B][6] = (stat, eq, ineq, bnd, compl, sign):
 *     stat   inf-norm of grad_lag
 *     eq     largest |g_i| over the equality rows (initial block, defects)
 *     ineq   largest violation lbg_i - g_i of an inequality row (pad, pair, obstacle), at least 0
 *     bnd    largest violation of a variable bound, at least 0
 *     compl  largest of |lam_g_i| (g_i - lbg_i) over the inequality rows and of max(-lam_x_j, 0) (w_j - lbx_j), max(lam_x_j, 0) (ubx_j - w_j)
 *            over the finite variable bounds, at least 0
 *     sign   largest positive lam_g_i on an inequality row (all are bounded below), at least 0
 *   A NaN in the inputs reaches the numbers it enters.  (obs, obs_stages) as above.  Works on every handle, like nmpc_eval_batch.
 */
typedef struct nmpc_duals { double *lam_g, *lam_x, *lam_p; } nmpc_duals_t;   /* device, each may be NULL */
int32_t nmpc_solve_batch_duals(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w0, double *w_out,
                               double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order, const nmpc_duals_t *duals, void *stream);
int32_t nmpc_step_batch_duals(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *obs, int32_t obs_stages, double *obj,
                              int32_t *status, int32_t *iters, double *kkt, int32_t *order, const nmpc_duals_t *duals, void *stream);
int32_t nmpc_kkt_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                       const double *lam_x, double *res /* [B][6] */, double *grad_lag /* [B][n_var] or NULL */, void *stream);

/*
 * Plan sensitivities and feedback gains: how the plan moves when the measured state or the goal moves, d w* / d p, and its first block
 * d U_0* / d x0 — the linear feedback around a plan that runs between two solves, and the correction of advanced-step NMPC.
 *
 * Definition: the linearisation of the solver's own barrier KKT system at a given primal-dual point.  Inputs (p, w, lam_g, lam_x) in the
 * layouts and the sign convention above (a solve's outputs, or any others), (obs, obs_stages) by the rules of nmpc_kkt_batch.  W is
 *   the exact Lagrangian Hessian grad^2 f + sum_i lam_g,i grad^2 g_i (2 Q, 2 R, the heading / speed curvature of the defects, the pair and
 *   obstacle blocks)
 *   + for every inequality row of stages 1..N-1: grad g_i Sigma_i grad g_i' with Sigma_i = z_i / s_i, z_i = max(-lam_g,i, 0), s_i = g_i - lbg_i
 *   + for every finite variable bound of X_1..X_N and U: max(lam_x, 0) / (ub - w) + max(-lam_x, 0) / (w - lb) on the diagonal;
 *   the pair and obstacle rows of stage 0, the pad rows and X_0 carry nothing (the structural zeros of the multipliers above).
 * The equality rows are the initial block and the defects, linearised: dX_0 = dx0, dX_{k+1} = A_k dX_k + B_k dU_k.  For dp = [dx0; dxs],
 * dw minimises 1/2 dw' W dw - sum_{k<N} (2 Q dxs)' dX_k on those equalities.  At a converged point this is the derivative of the barrier
 * solution at the solver's final mu: O(mu) from the NLP's own derivative wherever the NLP has one (where the active set changes it has none).
 * Solved by the stage recursion P_N = the bound terms of X_N, F = [F_uu F_ux; F_xu F_xx] = W_k + [B A]' P_{k+1} [B A], G_k = -F_uu^-1 F_ux,
 * without an inertia shift.
 *   gains [B][S][n_u][n_x]  S = gain_stages, 1 or N: G_k = d U_k / d X_k along the plan, G_0 = d U_0* / d x0; S = 1 writes stage 0 only
 *   dw    [B][n_var]        for dp [B][n_p]: dU_k = G_k dX_k + g_k, dX_0 = dx0 (copied)
 *   info  [B]               0: success.  1: some F_uu has a pivot <= 0 — the point is not a strict minimiser of its barrier problem.
 *                           2: a row or bound with a positive multiplier has s <= 0 (this verdict goes first).  With 1 or 2 the instance's
 *                           gains and dw are written as zeros.
 * gains and dw may each be NULL; dp == NULL requires dw == NULL; both NULL still computes info.  Saturated controls give gains near zero, a
 * swarm pressed against a pair row large ones.
 * Returns NMPC_E_ARG for null p, w, lam_g, lam_x or info with B > 0, gain_stages neither 1 nor N with gains != NULL, dw without dp, B beyond
 * max_batch, and the field errors of the *_obs calls; NMPC_E_UNSUPPORTED on handles that run on kernel 1 or 2, as the *_duals calls (they
 * cannot produce the multipliers either).  The inputs are read-only; the call is stream-ordered with the handle's other calls and uses the
 * handle's workspace between its two passes (the one-handle-one-stream rule above covers it); no solve result depends on it.
 */
int32_t nmpc_sens_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                        const double *lam_x, const double *dp, double *dw, double *gains, int32_t gain_stages, int32_t *info, void *stream);

/*
 * Adjoint plan sensitivities: the gradient of a scalar l(w*) with respect to the measured state, the goal and the per-instance obstacle field
 * from ONE launch, where the call above needs one launch per direction (n_p = 36 for six robots, N K 3 obstacle entries per instance).
 *
 * Notation as above: W is the barrier-augmented Lagrangian Hessian at (w, lam_g, lam_x), the equalities are the initial block and the
 * linearised defects, and S_p : dp -> dw is the map nmpc_sens_batch defines.  The obstacle map S_o : dobs -> dw, for a change dobs [S][K][3] of
 * the instance's field: dw minimises 1/2 dw' W dw + (M_o dobs)' dw on the homogeneous equalities (dX_0 = 0, linearised defects).  M_o collects
 * one contribution per obstacle row i = (k, robot, o) of stages k = 1..N-1 (the rows of stage 0 carry nothing, as everywhere else).  With e the
 * obstacle's entry at stage k (entry k when S == N, entry 0 when S == 1), ex = x - e.ox, ey = y - e.oy, rr = sqrt(ex^2 + ey^2), n = (ex, ey) / rr,
 * l = lam_g,i, s = rr - rob_dim - e.r - margin and Sigma = max(-l, 0) / s, the block of M_o in rows (x, y) of that robot at stage k is
 *   columns (ox, oy):  -l (I - n n') / rr - Sigma n n'
 *   column r:          -Sigma n
 * — d/do of the barrier stationarity condition, lam d_o grad g + grad g Sigma d_o g with d_o g = (-n', -1).
 *
 * For a cotangent wbar [B][n_var] of the plan the call returns the transposes:
 *   pbar   [B][n_p]      = S_p' wbar   (x0 half, then xs half)
 *   obsbar [B][S][K][3]  = S_o' wbar   S = obs_stages of the call; S == 1 sums the stages that share entry 0; entry 0 is exactly zero when S == N
 *   info   [B]           the verdicts of nmpc_sens_batch (2 first, then 1); with 1 or 2 the instance's outputs are zeros
 * Equivalently: let v minimise 1/2 v' W v - wbar' v on the homogeneous equalities; then pbar_xs = sum_{k<N} 2 Q v_{X_k}, obsbar = -M_o' v, and
 * pbar_x0 is the multiplier of that QP's initial block (minus the affine part of the stage-0 cost-to-go of the backward recursion).  The
 * defining identity is <pbar, dp> = <wbar, S_p dp> for every dp, and <obsbar, dobs> = <wbar, S_o dobs> for every dobs.  Sums over robots that
 * share an obstacle and over stages that share an entry run in a fixed order: the same inputs give the same bits.
 *
 * pbar and obsbar may each be NULL (both NULL still computes info).  obsbar != NULL with obs == NULL is NMPC_E_ARG: the handle's own field is
 * not a per-instance parameter.  The other argument errors are those of nmpc_sens_batch (null p, w, lam_g, lam_x, wbar or info with B > 0,
 * B beyond max_batch, the field errors of the *_obs calls), NMPC_E_UNSUPPORTED on handles that run on kernel 1 or 2.  The inputs are
 * read-only; the call is stream-ordered with the handle's other calls and uses the handle's workspace between its two passes exactly as
 * nmpc_sens_batch does (nmpc_workspace_bytes does not change); no solve result depends on it.
 */
int32_t nmpc_sens_adjoint_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                                const double *lam_x, const double *wbar, double *pbar, double *obsbar, int32_t *info, void *stream);

/*
 * Forward plan update: the first-order change of the plan when the measured state, the goal AND the per-instance obstacle field move between a
 * solve and its use, dw = S_p dp + S_o dobs in one launch, with a step limit alpha that says how much of it keeps every linearised slack
 * non-negative — the correction of advanced-step NMPC among moving obstacles.
 *
 * Notation as above.  (p, obs, obs_stages, w, lam_g, lam_x), W, the equalities, the verdicts (2 first, then 1) and the handle rules are exactly
 * those of nmpc_sens_batch.  dw minimises 1/2 dw' W dw + c' dw subject to dX_0 = dx0 and the linearised defects, with the linear term
 *   c = -2 Q dxs on X_k, k < N   +   M_o dobs   -   rhs
 *   dp   [B][n_p]        = [dx0; dxs]
 *   dobs [B][S][K][3]    S = obs_stages of the call: the change of the instance's field
 *   rhs  [B][n_var]      a general linear term
 * each may be NULL, which means zero.  M_o is the matrix defined under nmpc_sens_adjoint_batch: stage 0 carries nothing, entry 0 of a per-stage
 * dobs is not read, and with S == 1 entry 0 acts at every stage 1..N-1.  With dobs == rhs == NULL the call defines the dw of nmpc_sens_batch;
 * with only rhs = wbar it is the v of the adjoint call's text (pbar_xs = sum_{k<N} 2 Q v_{X_k}, obsbar = -M_o' v).  The terms of c at one entry
 * are added in a fixed order — goal, then rhs, then the obstacles in index order: the same inputs give the same bits.
 *   dw    [B][n_var]     dX_0 = dx0 (copied), dU_k = G_k dX_k + g_k along the linearised defects
 *   alpha [B]            the largest a in (0, 1] for which every linearised slack stays non-negative along a (dw, dobs):
 *                        alpha = min(1, min_i s_i / (-ds_i)) over the items with s_i > 0 and ds_i < 0.  The items are the pair and obstacle rows
 *                        of stages 1..N-1 and both sides of every finite bound of X_1..X_N and U_0..U_{N-1}:
 *                          pair row (i, a):   s = |xy_i - xy_a|^2 - d_min^2 with e = xy_i - xy_a,   ds = 2 e' (dxy_i - dxy_a)
 *                          obstacle row:      s = rr - rob_dim - e.r - margin,                      ds = n' (dxy - doxy) - dr   (that stage's entry of dobs)
 *                          upper bound:       s = ub - v,   ds = -dv;      lower bound:  s = v + ub,   ds = dv
 *                        Left out: the rows of stage 0, the pad rows, X_0 and the items with s_i <= 0 (nmpc_kkt_batch reports those).
 *                        alpha == 1.0 exactly when nothing limits the step.  No clipping of w + dw is done anywhere.
 *   info  [B]            the verdicts of nmpc_sens_batch; with 1 or 2 the instance gets dw = 0 and alpha = 0
 * dw and alpha may each be NULL (both NULL still computes info); each keeps its bits when the other is left out.
 * dobs != NULL with obs == NULL is NMPC_E_ARG: the handle's own field is not a per-instance parameter.  The other argument errors are those of
 * nmpc_sens_batch (null p, w, lam_g, lam_x or info with B > 0, B beyond max_batch, the field errors of the *_obs calls), NMPC_E_UNSUPPORTED on
 * handles that run on kernel 1 or 2.  The inputs are read-only; the call is stream-ordered with the handle's other calls and uses the handle's
 * workspace between its two passes exactly as nmpc_sens_batch does (nmpc_workspace_bytes does not change); no solve result depends on it.
 */
int32_t nmpc_sens_update_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                               const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw, double *alpha, int32_t *info,
                               void *stream);

/*
 * Forward plan update with its multiplier updates: nmpc_sens_update_batch, followed on the same stream by the dlam that go with its dw — the
 * corrected plan w + a dw keeps multipliers lam + a dlam, so nmpc_kkt_batch can certify it at the moved parameters (stationarity of second
 * order in the move), and nmpc_sens_* can linearise again at the corrected point without a re-solve.
 *
 * Notation as above: grad_lag = grad f + J' lam_g + lam_x as in nmpc_kkt_batch, H the exact Lagrangian Hessian, Sigma_i = max(-lam_g,i, 0) / s_i,
 * beta_j the bound term on W's diagonal, c the linear term of nmpc_sens_update_batch.  (dw, dlam_g, dlam_x) solve the linearised barrier KKT
 * system at fixed complementarity products:
 *   (a) stationarity:   H dw + J' dlam_g + dlam_x + (d_p grad_lag) dp + (d_obs grad_lag) dobs - rhs = 0, with (d_p grad_lag) dp = -2 Q dxs on every
 *                       X_k, k < N, and (d_obs grad_lag) dobs = sum_i lam_g,i d_o grad g_i dobs over the obstacle rows of stages 1..N-1;
 *   (b) equality rows:  dX_0 = dx0 and the linearised defects — the dw of nmpc_sens_update_batch;
 *   (c) inequality rows of stages 1..N-1:  dlam_g,i = Sigma_i ds_i with the ds_i of alpha's items (pair row: 2 e' (dxy_i - dxy_a); obstacle row:
 *                       n' (dxy - doxy) - dr, that stage's entry of dobs); exactly 0.0 on the rows of stage 0, on the pad rows and where lam_g,i >= 0;
 *   (d) bounds:         dlam_x,j = beta_j dw_j on X_1..X_N and U; exactly 0.0 on X_0, on an unbounded heading and where lam_x,j == 0;
 *   (e) initial block and defect rows: the multipliers of the QP's equalities, the unique values with which (a) holds on the rows of X.  With
 *                       the defect row g_k = X_{k+1} - (X_k + T f) and r = W dw + c:  dnu_{N-1} = -r_XN,  dnu_{k-1} = A_k' dnu_k - r_Xk,
 *                       dnu_init = A_0' dnu_0 - r_X0.
 *   dlam_g     [B][n_g]    (c) and (e)
 *   dlam_x     [B][n_var]  (d)
 *   alpha_dual [B]         the largest a in (0, 1] that keeps every multiplier's sign: min(1, min_i z_i / (-dz_i)) over the items with z_i > 0 and
 *                          dz_i < 0 — the inequality rows of (c) with z = -lam_g, dz = -dlam_g, and the bounds of (d) with z = |lam_x|,
 *                          dz = sign(lam_x) dlam_x.  1.0 exactly when nothing limits it.
 * With verdict 1 or 2 the instance's dlam_g and dlam_x are zeros and alpha_dual = 0 (dw = 0 and alpha = 0 as above).  The change of the
 * multiplier of p, dlam_p, is an output of nmpc_sens_update_batch_multi_duals (below; D = 1 for one direction).
 * dlam_g, dlam_x and alpha_dual may each be NULL; dw, alpha and info are bit for bit those of nmpc_sens_update_batch on the same inputs (with all
 * three NULL this is that call), and every output keeps its bits when any of the others is left out.  The argument errors and handle rules are
 * those of nmpc_sens_update_batch.  nmpc_workspace_bytes does not change: the multipliers need no workspace; only a call that asks for them with
 * dw == NULL makes the handle keep a [max_batch][n_var] buffer of its own for dw from then on (NMPC_E_NOMEM when that fails).
 */
int32_t nmpc_sens_update_batch_duals(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w,
                                     const double *lam_g, const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw,
                                     double *alpha, double *dlam_g, double *dlam_x, double *alpha_dual, int32_t *info, void *stream);

/*
 * Forward plan update for D directions in one launch: nmpc_sens_update_batch applied to D directions (dp, dobs, rhs)_d at the same primal-dual
 * point (p, obs, obs_stages, w, lam_g, lam_x) of every instance — the columns of the plan's Jacobian dw / dp or dw / dobs, the corrections of one
 * prepared plan for D candidate measurements or obstacle fields, D right-hand sides against one linearisation.  The part of the stage recursion
 * that depends on the point only is done once, not D times.
 *   dp    [B][D][n_p]          = [dx0; dxs] of direction d
 *   dobs  [B][D][S][K][3]      S = obs_stages of the call
 *   rhs   [B][D][n_var]
 * each may be NULL, which means zero for every direction.
 *   dw    [B][D][n_var]        required
 *   alpha [B][D]               may be NULL; dw keeps its bits without it
 *   info  [B]                  one verdict per instance: it depends on the point, not on the direction
 * Per direction d the contract is that of nmpc_sens_update_batch, word for word: dw[b][d] minimises 1/2 dw' W dw + c_d' dw subject to
 * dX_0 = dx0_d and the linearised defects, with c_d = -2 Q dxs_d on X_k, k < N, + M_o dobs_d - rhs_d, the terms of c_d at one entry added in the
 * fixed order goal, rhs, obstacles in index order; alpha[b][d] is the step limit of (dw[b][d], dobs_d) over the same items, with the same items
 * left out, and exactly 1.0 when nothing limits the step; the verdicts are those of nmpc_sens_batch, 2 before 1, and with either all D
 * directions of the instance get dw = 0 and alpha = 0.  The bits of a direction's dw and alpha do not depend on D, on the slot d the direction
 * stands in, or on what the other directions hold; the same inputs give the same bits.  They agree with nmpc_sens_update_batch on the same
 * direction to rounding, not bit for bit: the two kernels are compiled separately.
 * 1 <= D <= NMPC_SENS_MAX_DIRS, else NMPC_E_ARG; dw == NULL is NMPC_E_ARG (dw is where the call keeps a direction's feed-forward terms between
 * its two passes).  The other argument errors are those of nmpc_sens_update_batch: null p, w, lam_g, lam_x or info with B > 0, B beyond
 * max_batch, the field errors of the *_obs calls, dobs without obs; NMPC_E_UNSUPPORTED on handles that run on kernel 1 or 2.  Every check is made
 * on the host before anything is launched.  The inputs are read-only; the call is stream-ordered with the handle's other calls and uses the
 * handle's workspace between its two passes exactly as nmpc_sens_batch does (nmpc_workspace_bytes does not change); no solve result depends on it.
 * The multiplier updates of the D directions: nmpc_sens_update_batch_multi_duals, below.
 */
#define NMPC_SENS_MAX_DIRS 64
int32_t nmpc_sens_update_batch_multi(nmpc_handle_t *h, int32_t B, int32_t D, const double *p, const double *obs, int32_t obs_stages, const double *w,
                                     const double *lam_g, const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw,
                                     double *alpha, int32_t *info, void *stream);

/*
 * Forward plan update for D directions with their multiplier updates: nmpc_sens_update_batch_multi, followed on the same stream by one launch
 * that gives every direction the dlam that go with its dw — each corrected scenario w + a dw[b][d] keeps multipliers lam + a dlam[b][d], so
 * nmpc_kkt_batch can certify it, nmpc_sens_* can linearise again at it, and it can become the base of a chained correction; with unit
 * directions the outputs are the columns of d lam* / d p and d lam* / d obs.  The walk that gives the multipliers eliminates nothing, and what
 * it needs of the point at a stage is formed once for the D directions.
 *   dlam_g     [B][D][n_g]
 *   dlam_x     [B][D][n_var]
 *   alpha_dual [B][D]
 * Per direction d the contract is (a)-(e) of nmpc_sens_update_batch_duals, word for word, with (dp, dobs, rhs)_d and dw[b][d]: the exact zeros
 * (the inequality rows of stage 0, the pad rows, rows with lam_g,i >= 0; X_0, an unbounded heading, lam_x,j == 0), the items of alpha_dual, and
 * alpha_dual == 1.0 exactly when nothing limits it.
 *   dlam_p     [B][D][n_p]     the change of lam_p as defined under nmpc_solve_batch_duals: the x0 part equals dlam_g[b][d][:n_x], bit for bit; the
 *                              xs part is 2 Q (sum_{k<N} dX_k - N dxs_d) with dX_k of dw[b][d], the sum taken in the order k = N-1, N-2, .., 0.
 * The call is nmpc_sens_update_batch_multi and then that launch: dw, alpha and info are bit for bit those of nmpc_sens_update_batch_multi on
 * the same inputs; with dlam_g, dlam_x, dlam_p and alpha_dual all NULL this is that call.  Each of the four may be NULL, and every output keeps
 * its bits when any of the others is left out.  With verdict 1 or 2 all D directions of the instance get zeros in dlam_g, dlam_x and dlam_p and
 * alpha_dual = 0 (dw = 0 and alpha = 0 as there).  The bits of a direction's outputs do not depend on D, on the slot d the direction stands in,
 * or on what the other directions hold; no atomics, the same inputs give the same bits.  They agree with nmpc_sens_update_batch_duals on the
 * same direction to rounding, not bit for bit: the kernels are compiled separately.
 * The argument errors and handle rules are those of nmpc_sens_update_batch_multi — D outside 1 .. NMPC_SENS_MAX_DIRS, dw == NULL, null p, w,
 * lam_g, lam_x or info with B > 0, B beyond max_batch, the field errors of the *_obs calls, dobs without obs: NMPC_E_ARG; handles that run on
 * kernel 1 or 2: NMPC_E_UNSUPPORTED — every one checked on the host before anything is launched, and nothing is written on an error.  B == 0
 * returns NMPC_OK.  The multipliers need no workspace: nmpc_workspace_bytes does not change.
 */
int32_t nmpc_sens_update_batch_multi_duals(nmpc_handle_t *h, int32_t B, int32_t D, const double *p, const double *obs, int32_t obs_stages, const double *w,
                                           const double *lam_g, const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw,
                                           double *alpha, double *dlam_g, double *dlam_x, double *dlam_p, double *alpha_dual, int32_t *info,
                                           void *stream);

/*
 * Pose references per stage: the cost and the KKT certificate of a trajectory-tracking problem.  The two calls below are nmpc_eval_batch(_obs) and
 * nmpc_kkt_batch with the pose reference of every instance given apart from p, one row for the horizon or one per stage (the tutorial
 * lineage of the scripts carries it as P = [x0; x_ref,1 .. x_ref,N]; AS/mpc_control_trajectory_tracking.py tracks a path on its SLSQP route):
 *   ref [B][S][n_x] fp64 device, S = ref_stages, 1 or N.
 *   Stage k's cost term (k = 0..N-1, at X_k) is (X_k - xs_k)' Q (X_k - xs_k) with xs_k row k when S == N and row 0 when S == 1.  The xs half of
 *   p is not read by these calls; the x0 half is read as always.
 * (obs, obs_stages): obs == NULL and obs_stages == 0 is the handle's own obstacle field, otherwise the per-instance field by the rules of the
 * *_obs calls.  The row layout, n_g and the bounds are those of the plain calls; g does not depend on the reference, and given ref equal to the
 * xs half of p (either S) the outputs are those of the plain calls.  In nmpc_kkt_batch_ref, grad f of stage k is 2 Q (X_k - xs_k): a point whose
 * multipliers certify it here is a KKT point of the tracking problem, whoever computed it.
 * Returns NMPC_E_ARG when ref == NULL with B > 0, when ref_stages is neither 1 nor N, or for the argument errors of the *_obs calls.  Both
 * work on every handle, like nmpc_eval_batch.
 *
 * The tracking solve.  nmpc_solve_batch_ref / nmpc_step_batch_ref are nmpc_solve_batch_duals / nmpc_step_batch_duals with the cost of stage k
 * measured against row k of ref (the same ref [B][S][n_x], S = ref_stages, 1 or N, and the same stage rule as above): the interior-point
 * iteration, its rescue ladder, the status codes, the bounds and NMPC_STATUS_INFEASIBLE_X0 are those of the plain solve, and only the gradient
 * 2 Q (X_k - xs_k) of the cost knows the stage.  The xs half of p is NOT read (it may hold anything, NaN included); the x0 half is read as always.
 *   (obs, obs_stages): obs == NULL and obs_stages == 0 is the handle's own obstacle field, otherwise the per-instance field by the rules of the
 *   *_obs calls.  order and duals may be NULL; duals follows the rules of the *_duals calls.
 *   Multipliers: the conventions of nmpc_solve_batch_duals with xs_k in place of xs: the initial block of lam_g carries 2 Q (X_0 - xs_0), and
 *   the xs part of lam_p is 2 Q sum_{k<N} (X_k - xs_k), summed in the same order: -lam_p[n_x:] is the sensitivity of the optimal cost to a
 *   common translation of every reference row.  The x0 part is as before.
 *   The step call shifts the plan and steps the plant exactly as nmpc_step_batch does; ref is not written: the caller supplies the next
 *   period's window of its path.
 * DEFINING PROPERTY: given ref rows all equal to the xs half of p, with S = 1 or S = N, w_out, obj, status, iters, kkt and the multipliers are
 * bit-identical to nmpc_solve_batch_duals on the same inputs.
 * The calls run the column-per-lane kernel's tracking instantiations (every shape, chosen by B and order as for a *_obs call): handles that run
 * on kernel 1 or 2 (a pin, or a horizon beyond the column kernel's LDS) get NMPC_E_UNSUPPORTED.  NMPC_E_ARG as for the two calls above and for
 * the *_duals calls.  The sensitivity calls (nmpc_sens_*) take no p-dependent cost term and run unchanged at a tracking solution.
 */
int32_t nmpc_solve_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *ref, int32_t ref_stages, const double *obs, int32_t obs_stages,
                             const double *w0, double *w_out, double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order,
                             const nmpc_duals_t *duals, void *stream);
int32_t nmpc_step_batch_ref(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *ref, int32_t ref_stages, const double *obs,
                            int32_t obs_stages, double *obj, int32_t *status, int32_t *iters, double *kkt, int32_t *order, const nmpc_duals_t *duals,
                            void *stream);
int32_t nmpc_eval_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *w, const double *ref, int32_t ref_stages, const double *obs,
                            int32_t obs_stages, double *f, double *g, void *stream);
int32_t nmpc_kkt_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *ref, int32_t ref_stages, const double *obs, int32_t obs_stages,
                           const double *w, const double *lam_g, const double *lam_x, double *res, double *grad_lag /* [B][n_var] or NULL */, void *stream);

/*
 * Odometry front-end of the scripts' callbacks (AS/centralized_two_robots_implementation.py:18-37): for n robots,
 *   odom [n][4] = (x_r, y_r, q_z, q_w) wheel-odometry pose in the robot's own start frame (q_w is carried but, as in the
 *                  reference, not used: yaw = 2 asin(q_z)),
 *   init [n][3] = (x_init, y_init, th_init) pose of that start frame in the global frame,
 *   pose [n][3] = (x, y, phi) in the global frame: [x y] = R(th_init) [x_r y_r] + [x_init y_init], phi = th + th_init with
 *                  th = 2 asin(q_z), or, when wrap_2pi != 0, th = modify(2 asin(q_z)): the heading wrap into [0, 2 pi) of the
 *                  scripts without collision rows (AS/mpc_online_casadi.py:24-33: th in [-pi, 0) -> th + 2 pi); the collision-free
 *                  scripts' modify() is the identity (C2:62-68), i.e. wrap_2pi = 0.
 * Device pointers; no handle (pure function of its inputs).  SURVEY.md 8(f) row 3.
 */
int32_t nmpc_odometry_batch(int64_t n, const double *odom, const double *init, double *pose, int32_t wrap_2pi, void *stream);

/* library / kernel identification string: version, arch, and the hash of the sources it was built from (build.py) */
const char *nmpc_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NMPC_H_ */
