/*
 * nmpc_debug.h — development aids exported by libnmpc_hip.so next to the product ABI of nmpc.h.  Not part of the drop-in boundary:
 * nothing here has a counterpart in the reference, no product path calls it, and the layouts it exposes may change with the kernels.
 * Used by tools/ (phase profiles, per-iteration traces, workspace dumps of one instance).
 */
#ifndef NMPC_DEBUG_H_
#define NMPC_DEBUG_H_

#include "nmpc.h"
#include "nmpc_lidar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-phase cycle counters of a -DNMPC_PROFILE build: out12 [12] int64 (all zero in a product build); reset != 0 clears them */
int32_t nmpc_debug_profile(nmpc_handle_t *h, int64_t *out12, int32_t reset);
/* per-iteration trace of nmpc_options_t.trace_instance (NMPC_PROFILE builds): out [rows][16] doubles, rows <= 2048 */
int32_t nmpc_debug_trace(nmpc_handle_t *h, double *out, int32_t rows);
/* second trace block of the same instance: out [rows][8] doubles */
int32_t nmpc_debug_trace2(nmpc_handle_t *h, double *out, int32_t rows);
/* copies the per-instance workspace of one instance to the host; returns its length in doubles (out == NULL: length only);
   offs [5] (may be NULL) <- kernel, oKG, oKFF, oPACK, oKT */
int64_t nmpc_debug_workspace(nmpc_handle_t *h, int32_t inst, double *out, int64_t cap, int64_t *offs);


/* the kernel instantiation of one solve launch, as in its mangled name: solve_kernelILi{m}ELi{threads}E (kernel 1),
   solve_lds_kernelILi{m}ELi{thb}ELi{threads}E (2), solve_col_kernelILi{m}ELi{thb}ELi{flags}ELi{threads}E (3) */
typedef struct nmpc_debug_variant {
    int32_t kernel;        /* 1 HBM-resident, 2 element-per-lane, 3 column-per-lane */
    int32_t m, thb;        /* template team size, heading-bound flag (0 for kernel 1, which has no such template argument) */
    int32_t flags;         /* column kernel: the DL template argument exactly as instantiated (0/1/2, | 4 with the per-instance field); else 0 */
    int32_t threads;       /* workgroup size = TPB template argument */
    int64_t lds_bytes;     /* dynamic LDS of the launch */
} nmpc_debug_variant_t;
/* the instantiation a solve of B instances on this handle would launch (ordered != 0: with a dispatch-order hint; obs_field != 0: an *_obs call).
   No launch is made.  Returns NMPC_OK, NMPC_E_ARG, or NMPC_E_UNSUPPORTED where the call itself would. */
int32_t nmpc_debug_variant(const nmpc_handle_t *h, int32_t B, int32_t ordered, int32_t obs_field, nmpc_debug_variant_t *out);
/* the same without a handle and without a device: the instantiation the handle nmpc_create_opts(cfg, max_batch >= B, opts) makes on a device
   with compute_units compute units would launch, by the functions the handle itself chooses with.  *kernel (may be NULL) <- the kernel code
   NMPC_QUERY_KERNEL_FOR_BATCH / _ORDERED_BATCH answers (1..4).  Returns the codes of nmpc_debug_variant, and those of nmpc_create_opts for
   the configuration and the options (opts may be NULL). */
int32_t nmpc_debug_variant_of_config(const nmpc_config_t *cfg, const nmpc_options_t *opts, int32_t compute_units, int32_t B, int32_t ordered,
                                     int32_t obs_field, nmpc_debug_variant_t *out, int32_t *kernel);

/* the same for the tracking solve nmpc_solve_batch_ref (obs_field != 0: with obs): the row (3, m, thb, flags | 8, threads) of
   track_col_kernelILi{m}ELi{thb}ELi{flags}ELi{threads}E — flags in the name without the 8, always with the 4: the tracking kernel is instantiated
   with the per-instance field only — and its LDS bytes.  No launch is made; NMPC_E_UNSUPPORTED off the column kernel. */
int32_t nmpc_debug_track_variant_of_config(const nmpc_config_t *cfg, const nmpc_options_t *opts, int32_t compute_units, int32_t B, int32_t ordered,
                                           int32_t obs_field, nmpc_debug_variant_t *out, int32_t *kernel);

/* the kernel instantiation of one LIDAR solve launch (include/nmpc_lidar.h), as in its mangled name: lidar_solve_kernelILi{rays}ELi{waves}E */
typedef struct nmpc_debug_lidar_variant {
    int32_t rays;           /* template ray count: 10 (the scripts' count, loops unrolled for it) or -1 (any other count, predicated) */
    int32_t waves;          /* register budget: resident waves per SIMD the instantiation is compiled for, 1 or 2 */
    int32_t two_wave_above; /* the handle launches the two-wave build for B above this (4 x compute units); INT32_MAX where it never does (rays = -1) */
    int32_t threads;        /* workgroup size: one wavefront per robot */
    int64_t lds_bytes;      /* dynamic LDS of the launch */
} nmpc_debug_lidar_variant_t;
/* the instantiation nmpc_lidar_solve_batch() of B instances on this handle would launch, chosen by the function the call itself launches by.
   No launch is made.  Returns NMPC_OK, or NMPC_E_ARG where the call itself would (null handle, B outside 0..max_batch) or out is null. */
int32_t nmpc_debug_lidar_variant(const nmpc_lidar_handle_t *h, int32_t B, nmpc_debug_lidar_variant_t *out);

#ifdef __cplusplus
}
#endif
#endif /* NMPC_DEBUG_H_ */
