// nmpc_api.cpp — the C ABI of include/nmpc.h on top of the gfx950 kernels.
//
// There is deliberately no CPU fallback in this library: every entry point either runs the
// HIP kernels or returns an error code.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "nmpc_device.h"
#include "../../include/nmpc_debug.h"

// What create decides about the solve kernels of one configuration: pure arithmetic on (filled KParams, pin, compute units), no HIP call.
// solve_plan() maps it and a call to the launch.
struct Selector {
    int pin;              // nmpc_options_t.kernel: 0 chosen per call, 1 / 2 / 3 that kernel, 4 / 5 the column kernel's latency shape with two / four wavefronts
    int base;             // KERN_HBM / KERN_LDS / KERN_COL: the pin, or the column kernel, after the fallbacks for horizons beyond the LDS
    bool lds_fits;        // the element-per-lane kernel fits the LDS for this configuration
    bool lat_fits;        // the column kernel's latency shape (two wavefronts per instance, duals in LDS up to six robots) fits the LDS
    int32_t lat_slots;    // instances of that shape the device holds at once
    int32_t lat_slots4;   // the same for four wavefronts per instance (2 per CU at 256 VGPRs per wave)
};
// the launch of one solve call: kernel code (KERN_*: what NMPC_QUERY_KERNEL_FOR_BATCH answers), the column kernel's shape and the instantiation
struct SolvePlan {
    int kernel, shape;
    nmpc::SolveVariant v;
};

struct nmpc_handle {
    nmpc_config_t cfg;
    nmpc::KParams P;
    Selector sel;
    int32_t max_batch;
    double *ws;          // device workspace: max_batch * stride doubles
    int64_t ws_bytes;
    long long *prof;     // device counters of the NMPC_PROFILE build (12 x int64), else unused
    int device;          // device the workspace lives on; made current for the duration of every call
    int32_t *ord_chk;    // [max_batch + 1] permutation check of a dispatch-order hint: counts, then the "bad" flag
    int32_t *it_buf;     // [max_batch] iteration counts of nmpc_step_batch when the caller passes iters == NULL
    int32_t *st_buf;     // [max_batch] statuses of nmpc_step_batch when the caller passes status == NULL (the in-place update skips failed instances)
    double *cfg_field;   // [n_obs][3] device copy of the config's obstacle field: what a tracking solve without obs reads as its per-instance field (stride 0); nullptr without obstacles
    double *dw_buf;      // [max_batch][n_var] the dw that nmpc_sens_update_batch_duals computes its multipliers from when the caller passes dw == NULL; allocated by the first such call
};

// makes the handle's device current for one call and restores the caller's on return
struct DeviceScope {
    int prev = -1; bool ok = true, switched = false;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; switched = ok; }
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

static bool m_supported(int m) { return m >= 1 && m <= NMPC_MAX_ROBOTS; }      // every team size 1..10 is instantiated (7 and 9 since round 4)
using nmpc::KERN_HBM; using nmpc::KERN_LDS; using nmpc::KERN_COL; using nmpc::KERN_COL_LAT;
using nmpc::SHAPE_TP; using nmpc::SHAPE_LAT2; using nmpc::SHAPE_LAT4;
static const size_t LDS_PER_CU = (size_t)160 * 1024;

extern "C" {

int32_t nmpc_n_var(const nmpc_config_t *c) { return c ? 3 * c->m * (c->N + 1) + 2 * c->m * c->N : NMPC_E_ARG; }
int32_t nmpc_n_p(const nmpc_config_t *c) { return c ? 6 * c->m : NMPC_E_ARG; }
int32_t nmpc_n_g(const nmpc_config_t *c)
{
    if (!c) return NMPC_E_ARG;
    int M = c->pair_rows ? c->m * (c->m - 1) / 2 : 0;
    return 3 * c->m + (c->pad_rows ? M : 0) + (3 * c->m + M + c->m * c->n_obs) * c->N;
}

void nmpc_config_default(nmpc_config_t *c, int32_t m, int32_t N)
{
    memset(c, 0, sizeof(*c));
    c->m = m; c->N = N; c->n_obs = 0; c->pad_rows = m > 1;
    c->T = 0.05; c->dmin = 0.15;
    c->q[0] = 1.0; c->q[1] = 5.0; c->q[2] = 0.1;
    c->r[0] = 0.5; c->r[1] = 0.05;
    c->v_max = 0.22; c->w_max = 2.84; c->xy_max = 10.0; c->th_max = INFINITY;
    c->rob_dim = 0.2; c->margin = 0.1; c->pad_value = 3.5;
    c->tol = 1e-8; c->mu_init = 0.5; c->max_iter = 2000; c->pair_rows = 1;
}

static void fill_params(const nmpc_config_t *c, nmpc::KParams *P)
{
    memset(P, 0, sizeof(*P));
    const int m = c->m, N = c->N, nx = 3 * m, nu = 2 * m, M = c->pair_rows ? m * (m - 1) / 2 : 0, K = c->n_obs;
    P->m = m; P->N = N; P->K = K; P->pairs = (c->pair_rows && m > 1) ? 1 : 0;
    P->thb = isfinite(c->th_max) ? 1 : 0;
    P->nxb = m * (P->thb ? 3 : 2);
    P->nh = 2 * nu + 2 * P->nxb + M + m * K;
    P->o_ul = 0; P->o_uu = nu; P->o_xl = 2 * nu; P->o_xu = P->o_xl + P->nxb; P->o_pr = P->o_xu + P->nxb; P->o_ob = P->o_pr + M;
    P->n_ineq = N * 2 * nu + N * 2 * P->nxb + (N - 1) * (M + m * K);
    P->nvar = nmpc_n_var(c); P->ng = nmpc_n_g(c);
    P->rows0 = nx + (c->pad_rows ? M : 0); P->rowsk = nx + M + m * K;
    P->pad_rows = c->pad_rows; P->pad_value = c->pad_value; P->max_iter = c->max_iter;
    P->T = c->T; P->dmin2 = c->dmin * c->dmin; P->vmax = c->v_max; P->wmax = c->w_max; P->xymax = c->xy_max; P->thmax = c->th_max;
    P->robdim = c->rob_dim; P->margin = c->margin; P->tol = c->tol; P->mu_init = c->mu_init;
    P->rho_el = NMPC_ELASTIC_RHO;
    for (int d = 0; d < 3; d++) P->q[d] = c->q[d];
    for (int d = 0; d < 2; d++) P->r[d] = c->r[d];
    memcpy(P->obs, c->obs, sizeof(P->obs));
    // workspace carve-up; every array starts on a 128-byte boundary
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t at = o; o += (n + 15) / 16 * 16; return (int32_t)at; };
    const int64_t nX = (int64_t)(N + 1) * nx, nU = (int64_t)N * nu, nH = (int64_t)(N + 1) * P->nh;
    P->oX = take(nX); P->oU = take(nU); P->oLAM = take(nX); P->oS = take(nH); P->oZ = take(nH);
    P->oDX = take(nX); P->oDU = take(nU); P->oLAMN = take(nX); P->oDS = take(nH); P->oDZ = take(nH);
    P->oSN = take((int64_t)N * m); P->oCS = take((int64_t)N * m); P->oC = take(nX); P->oH = take(nH); P->oGX = take(nX);
    P->oHUU = take(nU); P->oGU = take(nU); P->oHVT = take((int64_t)N * m); P->oHTT = take((int64_t)N * m);
    P->oKG = take((int64_t)N * nu * nx); P->oKFF = take(nU);
    P->oEL = take(2 * nmpc::HbmWs::el_half(N, P->nh));  // elastic variables of the HBM-resident kernel and their steps (one per inequality slot; only the pair / obstacle slots are used)
    P->oCKP = take((int64_t)((N - 1) / NMPC_CKPT_EVERY + 1) * nmpc::HbmWs::ckpt_slot(nx));      // saved cost-to-go of the backward sweep (partial re-factorisation)
    P->stride = o;
    nmpc::lds_workspace_fill(P, m);
}

// the checks of nmpc_create_opts on a configuration and its options
static int32_t config_check(const nmpc_config_t *cfg, const nmpc_options_t *opts)
{
    if (opts && (opts->kernel < 0 || opts->kernel > 5)) return NMPC_E_ARG;
    if (cfg->N < 2 || cfg->N > 4096 || cfg->n_obs < 0 || cfg->n_obs > NMPC_MAX_OBSTACLES) return NMPC_E_ARG;
    if (!(cfg->T > 0.0) || !(cfg->v_max > 0.0) || !(cfg->w_max > 0.0) || !(cfg->xy_max > 0.0) || !(cfg->th_max > 0.0)) return NMPC_E_ARG;
    if (!(cfg->tol > 0.0) || !(cfg->mu_init > 0.0) || cfg->max_iter < 0) return NMPC_E_ARG;
    // weights: Q >= 0, R > 0 (a non-positive R makes every Quu indefinite: it would only surface as status 2 per instance);
    // distances and margins are lengths
    if (!(cfg->q[0] >= 0.0) || !(cfg->q[1] >= 0.0) || !(cfg->q[2] >= 0.0) || !(cfg->r[0] > 0.0) || !(cfg->r[1] > 0.0)) return NMPC_E_ARG;
    if (!(cfg->dmin >= 0.0) || (cfg->n_obs > 0 && (!(cfg->rob_dim >= 0.0) || !(cfg->margin >= 0.0)))) return NMPC_E_ARG;
    for (int o = 0; o < cfg->n_obs; o++) if (!(cfg->obs[3 * o + 2] >= 0.0)) return NMPC_E_ARG;
    if (cfg->pad_rows && !cfg->pair_rows) return NMPC_E_ARG;      // the padding rows only exist next to pair rows (C6:278)
    return m_supported(cfg->m) ? NMPC_OK : NMPC_E_UNSUPPORTED;
}

// cus: compute units of the device
static Selector selector_fill(const nmpc::KParams &P, int pin, int cus)
{
    Selector s;
    const int m = P.m;
    s.pin = pin;
    s.base = (pin >= 1 && pin <= 2) ? pin : KERN_COL;
    // horizons whose iterate does not fit the 160 KB of LDS of a CU run on the HBM-resident kernel (same algorithm, slower)
    if (s.base == KERN_COL && nmpc::col_kernel_bytes(P, m, SHAPE_TP) > LDS_PER_CU) s.base = KERN_LDS;
    const size_t lb = nmpc::col_kernel_bytes(P, m, SHAPE_LAT2), eb = nmpc::lds_kernel_bytes(P, m);
    s.lat_fits = lb > 0 && lb <= LDS_PER_CU;
    const int by_regs = m <= 6 ? 4 : 2, by_lds = s.lat_fits ? (int)(LDS_PER_CU / lb) : 0;
    s.lat_slots = cus * (by_lds < by_regs ? by_lds : by_regs);
    s.lat_slots4 = cus * (by_lds < 2 ? by_lds : 2);
    if (s.base == KERN_LDS && eb > LDS_PER_CU) s.base = KERN_HBM;
    s.lds_fits = eb <= LDS_PER_CU;
    return s;
}

// The launch a solve of B instances makes: which kernel, in which shape, and the instantiation (the select_* function of that kernel).
// solve_impl() launches by it; nmpc_query() and the nmpc_debug_variant* descriptors report it.  ordered: the call carries a dispatch-order
// hint; needs_column: it passes an obstacle field or asks for the multipliers, which only the column kernel serves; field: the instantiation
// reads the per-instance obstacle field; track: a tracking solve (the *_ref solve calls), which needs the column kernel and runs its tracking
// instantiation in the shape the same call without a reference would get.  false: the call is unsupported on this configuration (needs_column
// off the column kernel).
static bool solve_plan(const nmpc::KParams &P, const Selector &s, int32_t B, bool ordered, bool needs_column, bool field, SolvePlan *pl, bool track = false)
{
    needs_column = needs_column || track;
    if (needs_column && s.base != KERN_COL) return false;      // horizon beyond the column kernel's LDS, or a pin to kernel 1 / 2
    // Kernel.  The column-per-lane kernel (one wave per instance, two instances per SIMD up to six robots) is the
    // throughput path.  A batch that cannot fill those slots is a latency problem instead (the launch lasts as long as its longest
    // solve): there the element-per-lane kernel, one instance per SIMD and, for still smaller batches, 2-4 waves per instance, is
    // faster.  Measured (solves/s, column | element), six robots: B=256 14.7 k | 16.7 k, 512 28.6 k | 31.0 k, 1024 54.0 k | 46.4 k,
    // 2048 97 k | 89 k, 4096 164 k | 104 k, 8192 205 k | 131 k, 16384 251 k | 145 k; ten robots N=20: B=256 10.4 k | 11.9 k,
    // 512 13.1 k | 13.4 k, 1024 25.5 k | 23.0 k, 2048 41.5 k | 25.5 k, 4096 59 k | 27 k; N=30: B=256 3.4 k | 3.8 k, 512 5.7 k | 4.7 k.
    const int m = P.m;
    int kern = s.base;
    const bool own = s.base == KERN_COL && s.pin == 0;      // the column kernel, shape by batch size (pin 3: throughput shape always)
    // With a dispatch-order hint (long solves first: the receding-horizon loop, nmpc_step_batch) the latency shape pays up to four rounds of
    // instances — measured, six robots B=4096: sorted longest-first 15.5 ms against 18.4 ms in the throughput shape; warm closed loop 281 k
    // against 248 k solves/s — because the order keeps a long solve from starting in the last round
    if (ordered && own && s.lat_fits && m >= 4 && B <= 4 * s.lat_slots) kern = KERN_COL_LAT;
    else if (s.base == KERN_COL && s.pin >= 4) kern = s.lat_fits ? KERN_COL_LAT : KERN_COL;      // pinned to the column kernel's latency shape
    else if (own && s.lat_fits && m >= 4 && B <= 2 * s.lat_slots) {
        // The column kernel's latency shape (two wavefronts per instance) where the launch lasts as long as its longest solve.  It holds
        // lat_slots instances at once (4 per CU up to six robots: 256 VGPRs per wave; 2 per CU beyond; fewer when the LDS says so: the
        // composite's 63 KB with its duals make it 2 per CU = 512).
        // Measured, solves/s (throughput | latency shape): six robots B=512 34.6 k | 42.4 k, 1024 67 k | 83 k, 2048 122 k | 151 k, 4096 188 k | 174 k;
        // composite 512 13.2 k | 18.6 k, 1024 25.4 k | 28.7 k, 2048 43.4 k | 41.2 k; ten robots N=20 512 13.5 k | 16.0 k, 1024 26.5 k | 31.5 k,
        // 2048 49.5 k | 41.6 k; N=30 512 5.9 k | 6.9 k, 1024 11.2 k | 11.2 k.  Up to three robots a phase has no more than 64 items: nothing
        // for a second wave to do (two robots 1024: 457 k | 462 k).
        kern = KERN_COL_LAT;      // every measured crossover lies between two and four rounds of instances
    } else if (own && !s.lat_fits && s.lds_fits && ((m >= 8 && B <= 256) || (m >= 5 && m <= 6 && B <= 512)))
        kern = needs_column ? KERN_COL : KERN_LDS;      // a call that needs the column kernel keeps its throughput shape
    pl->kernel = kern;
    // latency shape: two wavefronts per instance, or four (pin 5; unpinned: five / six robots whose stage-parallel phases have more than 1000
    // items (obstacle rows: (N-1) m K) while the batch fits twice the instances that shape holds at once (2 per CU))
    const int64_t items = (int64_t)(P.N - 1) * m * P.K;
    pl->shape = kern != KERN_COL_LAT ? SHAPE_TP
                : s.pin == 4 ? SHAPE_LAT2
                : (s.pin == 5 || (m >= 5 && m <= 6 && items > 1000 && B <= 2 * s.lat_slots4)) ? SHAPE_LAT4 : SHAPE_LAT2;
    return kern == KERN_HBM   ? nmpc::select_solve(P, m, B, &pl->v)
           : kern == KERN_LDS ? nmpc::select_solve_lds(P, m, B, &pl->v)
           : track            ? nmpc::select_track_col(P, m, pl->shape, &pl->v)
                              : nmpc::select_solve_col(P, m, pl->shape, field, &pl->v);
}

int32_t nmpc_create(const nmpc_config_t *cfg, int32_t max_batch, nmpc_handle_t **out) { return nmpc_create_opts(cfg, max_batch, nullptr, out); }

// the device side of nmpc_create_opts on the zeroed handle; on an error the caller destroys it
static int32_t handle_init(nmpc_handle *h, const nmpc_config_t *cfg, int32_t max_batch, const nmpc_options_t *opts)
{
    if (hipGetDevice(&h->device) != hipSuccess) return NMPC_E_HIP;
    h->cfg = *cfg;
    fill_params(cfg, &h->P);
    h->max_batch = max_batch;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    h->sel = selector_fill(h->P, opts ? opts->kernel : 0, cus);
    const int64_t per = h->sel.base == KERN_HBM ? h->P.stride : h->P.stride2;
    h->ws_bytes = (int64_t)sizeof(double) * per * max_batch;
    if (hipMalloc((void **)&h->ws, (size_t)h->ws_bytes) != hipSuccess) return NMPC_E_NOMEM;
    if (hipMalloc((void **)&h->prof, (12 + 24 * 2048) * sizeof(long long)) != hipSuccess) return NMPC_E_NOMEM;
    (void)hipMemset(h->prof, 0, (12 + 24 * 2048) * sizeof(long long));
    if (hipMalloc((void **)&h->ord_chk, sizeof(int32_t) * ((size_t)max_batch + 1)) != hipSuccess) return NMPC_E_NOMEM;
    (void)hipMemset(h->ord_chk, 0, sizeof(int32_t) * ((size_t)max_batch + 1));
    if (hipMalloc((void **)&h->it_buf, sizeof(int32_t) * (size_t)max_batch) != hipSuccess) return NMPC_E_NOMEM;
    if (hipMalloc((void **)&h->st_buf, sizeof(int32_t) * (size_t)max_batch) != hipSuccess) return NMPC_E_NOMEM;
    h->P.trace_inst = opts ? opts->trace_instance : -1;
    if (cfg->n_obs > 0) {
        const size_t nb = sizeof(double) * 3 * (size_t)cfg->n_obs;
        if (hipMalloc((void **)&h->cfg_field, nb) != hipSuccess) return NMPC_E_NOMEM;
        if (hipMemcpy(h->cfg_field, cfg->obs, nb, hipMemcpyHostToDevice) != hipSuccess) return NMPC_E_HIP;
    }
    return NMPC_OK;
}

int32_t nmpc_create_opts(const nmpc_config_t *cfg, int32_t max_batch, const nmpc_options_t *opts, nmpc_handle_t **out)
{
    if (!cfg || !out || max_batch < 1) return NMPC_E_ARG;
    int32_t rc = config_check(cfg, opts);
    if (rc != NMPC_OK) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return NMPC_E_HIP;   // fail loudly: no CPU path exists
    nmpc_handle *h = (nmpc_handle *)calloc(1, sizeof(nmpc_handle));
    if (!h) return NMPC_E_NOMEM;
    rc = handle_init(h, cfg, max_batch, opts);
    if (rc != NMPC_OK) { nmpc_destroy(h); return rc; }
    *out = h;
    return NMPC_OK;
}

int32_t nmpc_destroy(nmpc_handle_t *h)
{
    if (!h) return NMPC_E_ARG;
    if (h->ws) (void)hipFree(h->ws);
    if (h->prof) (void)hipFree(h->prof);
    if (h->ord_chk) (void)hipFree(h->ord_chk);
    if (h->it_buf) (void)hipFree(h->it_buf);
    if (h->st_buf) (void)hipFree(h->st_buf);
    if (h->dw_buf) (void)hipFree(h->dw_buf);
    if (h->cfg_field) (void)hipFree(h->cfg_field);
    free(h);
    return NMPC_OK;
}

int64_t nmpc_workspace_bytes(const nmpc_handle_t *h) { return h ? h->ws_bytes : 0; }

// The checks every entry point with an obstacle-field argument starts with.  CK_BOUNDED: B may not exceed max_batch; CK_OPT_FIELD: (NULL, 0) =
// the handle's own field (the *_duals calls and nmpc_kkt_batch), else a per-instance field is required (obs may be NULL only for an empty
// batch); CK_COLUMN: the call needs the column kernel.
enum { CK_BOUNDED = 1, CK_OPT_FIELD = 2, CK_COLUMN = 4 };
static int32_t call_check(const nmpc_handle_t *h, int32_t B, const double *obs, int32_t obs_stages, int ck)
{
    if (!h || B < 0 || ((ck & CK_BOUNDED) && B > h->max_batch)) return NMPC_E_ARG;
    const bool own = (ck & CK_OPT_FIELD) && !obs && obs_stages == 0;
    if (!own && (h->cfg.n_obs == 0 || (obs_stages != 1 && obs_stages != h->cfg.N) || (B > 0 && !obs))) return NMPC_E_ARG;
    return ((ck & CK_COLUMN) && h->sel.base != KERN_COL) ? NMPC_E_UNSUPPORTED : NMPC_OK;
}

// the per-instance obstacle field [B][obs_stages][n_obs][3] of a call as the kernels read it
static void set_field(nmpc::KParams *P, const nmpc_config_t &cfg, const double *obs, int32_t obs_stages)
{
    P->ofield.ptr = obs;
    P->ofield.istride = obs_stages * cfg.n_obs * 3;
    P->ofield.sstride = obs_stages == 1 ? 0 : cfg.n_obs * 3;
}

// the pose reference of an eval / kkt call as the kernels read it: ref [B][ref_stages][n_x] of the *_ref entry points (checked by ref_check), or,
// ref == nullptr, the xs half of p
static nmpc::PoseRef pose_ref(const nmpc_config_t &cfg, const double *p, const double *ref, int32_t ref_stages)
{
    const int32_t nx = 3 * cfg.m;
    if (!ref) return nmpc::PoseRef{p + nx, 2 * nx, 0};
    return nmpc::PoseRef{ref, ref_stages * nx, ref_stages == cfg.N ? nx : 0};
}

// the checks of the *_ref entry points on their reference argument, after call_check
static int32_t ref_check(const nmpc_handle_t *h, int32_t B, const double *ref, int32_t ref_stages)
{
    return ((ref_stages != 1 && ref_stages != h->cfg.N) || (B > 0 && !ref)) ? NMPC_E_ARG : NMPC_OK;
}

static bool wants_duals(const nmpc_duals_t *d) { return d && (d->lam_g || d->lam_x || d->lam_p); }

// obs != NULL: the obstacle field of the instances, [B][obs_stages][n_obs][3] (checked by call_check), read by the column kernel's
// per-instance field instantiations; handles that run on kernel 1 or 2 have none.  duals: the multiplier outputs of the *_duals entry points,
// written by the column kernel's epilogue (nullptr, or all members nullptr: the plain call).  ref != NULL: the tracking solve, ref
// [B][ref_stages][n_x] (checked by ref_check) read by the column kernel's tracking instantiations, which exist with the per-instance field only:
// without obs every instance reads the handle's device copy of the config's field
static int32_t solve_impl(nmpc_handle_t *h, int32_t B, const double *p, const double *w0, double *w_out, double *obj, int32_t *status,
                          int32_t *iters, double *kkt, const int32_t *order, void *stream, const double *obs = nullptr, int32_t obs_stages = 0,
                          const nmpc_duals_t *duals = nullptr, const double *ref = nullptr, int32_t ref_stages = 0)
{
    if (!h || B < 0 || B > h->max_batch) return NMPC_E_ARG;
    const bool du = wants_duals(duals);
    SolvePlan pl;
    if (!solve_plan(h->P, h->sel, B, order != nullptr, obs || du, obs != nullptr, &pl, ref != nullptr)) return NMPC_E_UNSUPPORTED;
    if (B == 0) return NMPC_OK;      /* empty batch: nothing to read or write, pointers may be null */
    if (!p || !w0 || !w_out) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    P.order = order;
    P.order_bad = h->ord_chk + B;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    else if (ref) { P.ofield.ptr = h->cfg_field; P.ofield.istride = 0; P.ofield.sstride = 0; }
    if (du) { P.lam_g = duals->lam_g; P.lam_x = duals->lam_x; P.lam_p = duals->lam_p; }
    if (order && nmpc::launch_order_check(B, order, h->ord_chk, h->ord_chk + B, (hipStream_t)stream) != hipSuccess) return NMPC_E_HIP;
    const nmpc::SolveArgs a{p, w0, w_out, obj, status, iters, kkt, h->ws, h->prof, ref ? pose_ref(h->cfg, p, ref, ref_stages) : nmpc::PoseRef{nullptr, 0, 0}};
    hipError_t e = pl.v.kernel == KERN_HBM   ? nmpc::launch_solve(P, pl.v, B, a, (hipStream_t)stream)
                   : pl.v.kernel == KERN_LDS ? nmpc::launch_solve_lds(P, pl.v, B, a, (hipStream_t)stream)
                                             : nmpc::launch_solve_col(P, pl.v, B, a, (hipStream_t)stream);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_solve_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *w0, double *w_out, double *obj, int32_t *status,
                         int32_t *iters, double *kkt, void *stream)
{
    return solve_impl(h, B, p, w0, w_out, obj, status, iters, kkt, nullptr, stream);
}

int32_t nmpc_solve_batch_ordered(nmpc_handle_t *h, int32_t B, const double *p, const double *w0, double *w_out, double *obj,
                                 int32_t *status, int32_t *iters, double *kkt, const int32_t *order, void *stream)
{
    return solve_impl(h, B, p, w0, w_out, obj, status, iters, kkt, order, stream);
}

static int32_t step_impl(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, double *obj, int32_t *status, int32_t *iters, double *kkt,
                         int32_t *order, void *stream, const double *obs = nullptr, int32_t obs_stages = 0, const nmpc_duals_t *duals = nullptr,
                         const double *ref = nullptr, int32_t ref_stages = 0)
{
    if (!h || B < 0 || B > h->max_batch) return NMPC_E_ARG;
    if ((obs || ref || wants_duals(duals)) && h->sel.base != KERN_COL) return NMPC_E_UNSUPPORTED;
    if (B == 0) return NMPC_OK;
    if (!p || !w || !w_sol || w == w_sol) return NMPC_E_ARG;
    int32_t *it = iters ? iters : h->it_buf;
    int32_t *stt = status ? status : h->st_buf;
    // 1. the solve, dispatched in the caller's order (checked to be a permutation; ignored otherwise)
    int32_t rc = solve_impl(h, B, p, w, w_sol, obj, stt, it, kkt, order, stream, obs, obs_stages, duals, ref, ref_stages);      // the multipliers of this period's w_sol
    if (rc != NMPC_OK) return rc;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    // 2. guess <- shift(solution) in place of the old guess; x0 <- x0 + T f(x0, u_0) in place of the x0 half of p.  An instance whose solve
    //    ended with status 2 (numerical failure: the iterate may be non-finite) or 3 (infeasible x0) keeps its guess and its x0;
    //    status 1 / 4 return a finite last iterate and are shifted like a converged one, as the scripts do with any IPOPT return
    if (nmpc::launch_shift(h->P, h->cfg.m, B, p, w_sol, w, p, 2 * 3 * h->cfg.m, stt, (hipStream_t)stream) != hipSuccess) return NMPC_E_HIP;
    // 3. the next period's dispatch order: longest solves of this period first
    if (order && nmpc::launch_order_by_iters(B, it, order, (hipStream_t)stream) != hipSuccess) return NMPC_E_HIP;
    return NMPC_OK;
}

int32_t nmpc_step_batch(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, double *obj, int32_t *status, int32_t *iters, double *kkt,
                        int32_t *order, void *stream)
{
    return step_impl(h, B, p, w, w_sol, obj, status, iters, kkt, order, stream);
}

int32_t nmpc_solve_batch_obs(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w0, double *w_out,
                             double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_COLUMN);
    return rc != NMPC_OK ? rc : solve_impl(h, B, p, w0, w_out, obj, status, iters, kkt, order, stream, obs, obs_stages);
}

int32_t nmpc_step_batch_obs(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *obs, int32_t obs_stages, double *obj,
                            int32_t *status, int32_t *iters, double *kkt, int32_t *order, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_COLUMN);
    return rc != NMPC_OK ? rc : step_impl(h, B, p, w, w_sol, obj, status, iters, kkt, order, stream, obs, obs_stages);
}

// the evaluation of f and g behind the three eval entry points, after their checks: obs (or nullptr: the handle's own field) and ref (or
// nullptr: the xs half of p) by the same rule
static int32_t eval_impl(nmpc_handle_t *h, int32_t B, const double *p, const double *w, const double *ref, int32_t ref_stages, const double *obs,
                         int32_t obs_stages, double *f, double *g, void *stream)
{
    if (B == 0) return NMPC_OK;
    if (!p || !w) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_eval(P, pose_ref(h->cfg, p, ref, ref_stages), h->cfg.m, B, p, w, f, g, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_eval_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *w, double *f, double *g, void *stream)
{
    if (!h || B < 0) return NMPC_E_ARG;
    return eval_impl(h, B, p, w, nullptr, 0, nullptr, 0, f, g, stream);
}

int32_t nmpc_eval_batch_obs(nmpc_handle_t *h, int32_t B, const double *p, const double *w, const double *obs, int32_t obs_stages, double *f, double *g,
                            void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, 0);
    return rc != NMPC_OK ? rc : eval_impl(h, B, p, w, nullptr, 0, obs, obs_stages, f, g, stream);
}

int32_t nmpc_solve_batch_duals(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w0, double *w_out,
                               double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order, const nmpc_duals_t *duals, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    return rc != NMPC_OK ? rc : solve_impl(h, B, p, w0, w_out, obj, status, iters, kkt, order, stream, obs, obs_stages, duals);
}

int32_t nmpc_step_batch_duals(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *obs, int32_t obs_stages, double *obj,
                              int32_t *status, int32_t *iters, double *kkt, int32_t *order, const nmpc_duals_t *duals, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    return rc != NMPC_OK ? rc : step_impl(h, B, p, w, w_sol, obj, status, iters, kkt, order, stream, obs, obs_stages, duals);
}

static int32_t kkt_impl(nmpc_handle_t *h, int32_t B, const double *p, const double *ref, int32_t ref_stages, const double *obs, int32_t obs_stages,
                        const double *w, const double *lam_g, const double *lam_x, double *res, double *grad_lag, void *stream)
{
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !res) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_kkt(P, pose_ref(h->cfg, p, ref, ref_stages), h->cfg.m, B, p, w, lam_g, lam_x, res, grad_lag, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_kkt_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                       const double *lam_x, double *res, double *grad_lag, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_OPT_FIELD);
    return rc != NMPC_OK ? rc : kkt_impl(h, B, p, nullptr, 0, obs, obs_stages, w, lam_g, lam_x, res, grad_lag, stream);
}

int32_t nmpc_sens_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                        const double *lam_x, const double *dp, double *dw, double *gains, int32_t gain_stages, int32_t *info, void *stream)
{
    // the column kernel's handles only: they produce the multipliers, and their workspace has the pivot-row region the two passes share
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if ((gains && gain_stages != 1 && gain_stages != h->cfg.N) || (dw && !dp)) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_sens(P, h->cfg.m, B, w, lam_g, lam_x, dw ? dp : nullptr, dw, gains, gain_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_sens_adjoint_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                                const double *lam_x, const double *wbar, double *pbar, double *obsbar, int32_t *info, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if (obsbar && !obs) return NMPC_E_ARG;      // the handle's own field is no per-instance parameter: it has no cotangent
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !wbar || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_sens_adjoint(P, h->cfg.m, B, w, lam_g, lam_x, wbar, pbar, obsbar, obs_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_sens_update_batch(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                               const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw, double *alpha, int32_t *info,
                               void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if (dobs && !obs) return NMPC_E_ARG;      // the handle's own field is no per-instance parameter: it has no change to give
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_sens_fwd(P, h->cfg.m, B, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, obs_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_sens_update_batch_duals(nmpc_handle_t *h, int32_t B, const double *p, const double *obs, int32_t obs_stages, const double *w, const double *lam_g,
                                     const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw, double *alpha,
                                     double *dlam_g, double *dlam_x, double *alpha_dual, int32_t *info, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if (dobs && !obs) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    const bool duals = dlam_g || dlam_x || alpha_dual;
    if (duals && !dw) {      // the multipliers follow from dw: it goes to the handle's own buffer, which the caller never sees
        if (!h->dw_buf && hipMalloc((void **)&h->dw_buf, sizeof(double) * (size_t)h->max_batch * (size_t)h->P.nvar) != hipSuccess) return NMPC_E_NOMEM;
        dw = h->dw_buf;
    }
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    // the update kernel exactly as nmpc_sens_update_batch launches it, then the multipliers from its dw and verdicts on the same stream
    hipError_t e = nmpc::launch_sens_fwd(P, h->cfg.m, B, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, obs_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    if (e == hipSuccess && duals)
        e = nmpc::launch_sens_dual(P, h->cfg.m, B, w, lam_g, lam_x, dp, dobs, rhs, dw, obs_stages, info, dlam_g, dlam_x, alpha_dual, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_sens_update_batch_multi(nmpc_handle_t *h, int32_t B, int32_t D, const double *p, const double *obs, int32_t obs_stages, const double *w,
                                     const double *lam_g, const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw,
                                     double *alpha, int32_t *info, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if (D < 1 || D > NMPC_SENS_MAX_DIRS || !dw) return NMPC_E_ARG;      // dw also carries each direction's feed-forward terms between the two passes
    if (dobs && !obs) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    hipError_t e = nmpc::launch_plan_dirs(P, h->cfg.m, B, D, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, obs_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_sens_update_batch_multi_duals(nmpc_handle_t *h, int32_t B, int32_t D, const double *p, const double *obs, int32_t obs_stages, const double *w,
                                           const double *lam_g, const double *lam_x, const double *dp, const double *dobs, const double *rhs, double *dw,
                                           double *alpha, double *dlam_g, double *dlam_x, double *dlam_p, double *alpha_dual, int32_t *info, void *stream)
{
    const int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc != NMPC_OK) return rc;
    if (D < 1 || D > NMPC_SENS_MAX_DIRS || !dw) return NMPC_E_ARG;
    if (dobs && !obs) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!p || !w || !lam_g || !lam_x || !info) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    nmpc::KParams P = h->P;
    if (obs) set_field(&P, h->cfg, obs, obs_stages);
    // the update kernel exactly as nmpc_sens_update_batch_multi launches it, then the multipliers from its dw and verdicts on the same stream
    hipError_t e = nmpc::launch_plan_dirs(P, h->cfg.m, B, D, w, lam_g, lam_x, dp, dobs, rhs, dw, alpha, obs_stages, info, h->ws, (hipStream_t)stream, obs != nullptr);
    if (e == hipSuccess && (dlam_g || dlam_x || dlam_p || alpha_dual))
        e = nmpc::launch_dual_dirs(P, h->cfg.m, B, D, w, lam_g, lam_x, dp, dobs, rhs, dw, obs_stages, info, dlam_g, dlam_x, dlam_p, alpha_dual, (hipStream_t)stream,
                                   obs != nullptr);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

/* ---- the *_ref entry points: a pose reference per instance, one row or one per stage, in place of the xs half of p */
int32_t nmpc_eval_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *w, const double *ref, int32_t ref_stages, const double *obs,
                            int32_t obs_stages, double *f, double *g, void *stream)
{
    int32_t rc = call_check(h, B, obs, obs_stages, CK_OPT_FIELD);
    if (rc == NMPC_OK) rc = ref_check(h, B, ref, ref_stages);
    return rc != NMPC_OK ? rc : eval_impl(h, B, p, w, ref, ref_stages, obs, obs_stages, f, g, stream);
}

int32_t nmpc_kkt_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *ref, int32_t ref_stages, const double *obs, int32_t obs_stages,
                           const double *w, const double *lam_g, const double *lam_x, double *res, double *grad_lag, void *stream)
{
    int32_t rc = call_check(h, B, obs, obs_stages, CK_OPT_FIELD);
    if (rc == NMPC_OK) rc = ref_check(h, B, ref, ref_stages);
    return rc != NMPC_OK ? rc : kkt_impl(h, B, p, ref, ref_stages, obs, obs_stages, w, lam_g, lam_x, res, grad_lag, stream);
}

int32_t nmpc_solve_batch_ref(nmpc_handle_t *h, int32_t B, const double *p, const double *ref, int32_t ref_stages, const double *obs, int32_t obs_stages,
                             const double *w0, double *w_out, double *obj, int32_t *status, int32_t *iters, double *kkt, const int32_t *order,
                             const nmpc_duals_t *duals, void *stream)
{
    int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc == NMPC_OK) rc = ref_check(h, B, ref, ref_stages);
    if (rc != NMPC_OK || B == 0) return rc;
    return solve_impl(h, B, p, w0, w_out, obj, status, iters, kkt, order, stream, obs, obs_stages, duals, ref, ref_stages);
}

int32_t nmpc_step_batch_ref(nmpc_handle_t *h, int32_t B, double *p, double *w, double *w_sol, const double *ref, int32_t ref_stages, const double *obs,
                            int32_t obs_stages, double *obj, int32_t *status, int32_t *iters, double *kkt, int32_t *order, const nmpc_duals_t *duals,
                            void *stream)
{
    int32_t rc = call_check(h, B, obs, obs_stages, CK_BOUNDED | CK_OPT_FIELD | CK_COLUMN);
    if (rc == NMPC_OK) rc = ref_check(h, B, ref, ref_stages);
    if (rc != NMPC_OK || B == 0) return rc;
    return step_impl(h, B, p, w, w_sol, obj, status, iters, kkt, order, stream, obs, obs_stages, duals, ref, ref_stages);
}

int32_t nmpc_shift_batch(nmpc_handle_t *h, int32_t B, const double *p_in, const double *w_in, double *w_next, double *x0_next, void *stream)
{
    if (!h || B < 0) return NMPC_E_ARG;
    if (B == 0) return NMPC_OK;
    if (!w_in || !w_next || w_in == w_next) return NMPC_E_ARG;
    if (x0_next && !p_in) return NMPC_E_ARG;
    DeviceScope dev(h->device);
    if (!dev.ok) return NMPC_E_HIP;
    hipError_t e = nmpc::launch_shift(h->P, h->cfg.m, B, p_in, w_in, w_next, x0_next, 0, nullptr, (hipStream_t)stream);
    return e == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int32_t nmpc_odometry_batch(int64_t n, const double *odom, const double *init, double *pose, int32_t wrap_2pi, void *stream)
{
    if (n < 0) return NMPC_E_ARG;
    if (n == 0) return NMPC_OK;
    if (!odom || !init || !pose) return NMPC_E_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return NMPC_E_HIP;
    return nmpc::launch_odometry((long)n, odom, init, pose, wrap_2pi != 0, (hipStream_t)stream) == hipSuccess ? NMPC_OK : NMPC_E_HIP;
}

int64_t nmpc_query(const nmpc_handle_t *h, int32_t what, int64_t arg)
{
    if (!h) return NMPC_E_ARG;
    SolvePlan pl;
    switch (what) {
    case NMPC_QUERY_KERNEL_FOR_BATCH:
    case NMPC_QUERY_KERNEL_FOR_ORDERED_BATCH:
    case NMPC_QUERY_LDS_BYTES:
        if (arg < 0 || arg > h->max_batch || !solve_plan(h->P, h->sel, (int32_t)arg, what == NMPC_QUERY_KERNEL_FOR_ORDERED_BATCH, false, false, &pl)) return NMPC_E_ARG;
        if (what != NMPC_QUERY_LDS_BYTES) return pl.kernel;
        return pl.kernel == KERN_LDS ? (int64_t)nmpc::lds_kernel_bytes(h->P, h->cfg.m) : (int64_t)pl.v.lds;      // kernel 2: its throughput shape's, whatever B
    case NMPC_QUERY_WORKSPACE_BYTES: return h->ws_bytes;
    case NMPC_QUERY_MAX_BATCH: return h->max_batch;
    case NMPC_QUERY_SENS_DIRS_PER_PASS: return nmpc::plan_dirs_per_pass(h->cfg.m);
    default: return NMPC_E_ARG;
    }
}

/* ---- development aids, declared in include/nmpc_debug.h (not part of the drop-in boundary) */
/* per-phase cycle counters of an NMPC_PROFILE build */
int32_t nmpc_debug_profile(nmpc_handle_t *h, int64_t *out12, int32_t reset)
{
    if (!h || !out12) return NMPC_E_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return NMPC_E_HIP;
    if (hipMemcpy(out12, h->prof, 12 * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return NMPC_E_HIP;
    if (reset) (void)hipMemset(h->prof, 0, 12 * sizeof(long long));
    return NMPC_OK;
}
int32_t nmpc_debug_trace(nmpc_handle_t *h, double *out, int32_t rows)
{
    if (!h || !out || rows < 0 || rows > 2048) return NMPC_E_ARG;
    if (rows == 0) return NMPC_OK;
    if (hipDeviceSynchronize() != hipSuccess) return NMPC_E_HIP;
    if (hipMemcpy(out, h->prof + 12, (size_t)rows * 16 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return NMPC_E_HIP;
    return NMPC_OK;
}
int32_t nmpc_debug_trace2(nmpc_handle_t *h, double *out, int32_t rows)
{
    if (!h || !out || rows < 0 || rows > 2048) return NMPC_E_ARG;
    if (rows == 0) return NMPC_OK;
    if (hipMemcpy(out, h->prof + 12 + 16 * 2048, (size_t)rows * 8 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return NMPC_E_HIP;
    return NMPC_OK;
}

/* copy the per-instance workspace of one instance to the host; returns its length in doubles */
int64_t nmpc_debug_workspace(nmpc_handle_t *h, int32_t inst, double *out, int64_t cap, int64_t *offs)
{
    if (!h) return NMPC_E_ARG;
    int64_t per = h->sel.base == KERN_HBM ? h->P.stride : h->P.stride2;
    if (offs) { offs[0] = h->sel.base; offs[1] = h->P.oKG; offs[2] = h->P.oKFF; offs[3] = h->P.oPACK; offs[4] = h->P.oKT; }
    if (!out) return per;
    if (cap < per || inst < 0 || inst >= h->max_batch) return NMPC_E_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return NMPC_E_HIP;
    if (hipMemcpy(out, h->ws + (size_t)inst * per, (size_t)per * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return NMPC_E_HIP;
    return per;
}

/* the descriptor of a plan, with the codes of the call it describes */
static int32_t describe(const nmpc_config_t &cfg, const nmpc::KParams &P, const Selector &sel, int32_t B, int32_t ordered, int32_t obs_field,
                        nmpc_debug_variant_t *out, int32_t *kernel, bool track = false)
{
    if (obs_field && cfg.n_obs == 0) return NMPC_E_ARG;      // as call_check()
    SolvePlan pl;
    if (!solve_plan(P, sel, B, ordered != 0, obs_field != 0, obs_field != 0, &pl, track)) return NMPC_E_UNSUPPORTED;
    const nmpc::SolveVariant &v = pl.v;
    out->kernel = v.kernel; out->m = v.m; out->thb = v.thb; out->flags = v.flags; out->threads = v.threads; out->lds_bytes = (int64_t)v.lds;
    if (kernel) *kernel = pl.kernel;
    return NMPC_OK;
}

/* the instantiation a solve of B instances on this handle would launch; no launch is made */
int32_t nmpc_debug_variant(const nmpc_handle_t *h, int32_t B, int32_t ordered, int32_t obs_field, nmpc_debug_variant_t *out)
{
    if (!h || !out || B < 0 || B > h->max_batch) return NMPC_E_ARG;
    return describe(h->cfg, h->P, h->sel, B, ordered, obs_field, out, nullptr);
}

/* the same for the handle nmpc_create_opts(cfg, >= B, opts) makes on a device with that many compute units; needs neither */
int32_t nmpc_debug_variant_of_config(const nmpc_config_t *cfg, const nmpc_options_t *opts, int32_t compute_units, int32_t B, int32_t ordered,
                                     int32_t obs_field, nmpc_debug_variant_t *out, int32_t *kernel)
{
    if (!cfg || !out || compute_units < 1 || B < 0) return NMPC_E_ARG;
    const int32_t rc = config_check(cfg, opts);
    if (rc != NMPC_OK) return rc;
    nmpc::KParams P;
    fill_params(cfg, &P);
    return describe(*cfg, P, selector_fill(P, opts ? opts->kernel : 0, compute_units), B, ordered, obs_field, out, kernel);
}

/* the same for a tracking solve (nmpc_solve_batch_ref) of B instances: the tracking row (3, m, thb, flags | 8, threads) and its LDS bytes */
int32_t nmpc_debug_track_variant_of_config(const nmpc_config_t *cfg, const nmpc_options_t *opts, int32_t compute_units, int32_t B, int32_t ordered,
                                           int32_t obs_field, nmpc_debug_variant_t *out, int32_t *kernel)
{
    if (!cfg || !out || compute_units < 1 || B < 0) return NMPC_E_ARG;
    const int32_t rc = config_check(cfg, opts);
    if (rc != NMPC_OK) return rc;
    nmpc::KParams P;
    fill_params(cfg, &P);
    return describe(*cfg, P, selector_fill(P, opts ? opts->kernel : 0, compute_units), B, ordered, obs_field, out, kernel, true);
}

#ifndef NMPC_SRC_HASH
#define NMPC_SRC_HASH "unknown"
#endif
const char *nmpc_version(void) { return "nmpc_hip 0.2 (gfx950, fp64, one wavefront per swarm instance) src=" NMPC_SRC_HASH; }

}  // extern "C"
