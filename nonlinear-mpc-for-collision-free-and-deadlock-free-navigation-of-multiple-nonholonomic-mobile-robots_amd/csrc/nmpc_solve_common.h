// nmpc_solve_common.h — what the three swarm solve kernels share (nmpc_kernels.hip: HBM-resident; nmpc_solve_lds.hip: element-per-lane Riccati
// stage; nmpc_solve_col.hip: column-per-lane, register-resident Riccati stage): the obstacle field, the simple bounds, the start / restart /
// exit text; and what the two LDS-resident ones share: the geometry of a stage (G2), the layout of their per-instance workspace (WsLayout: one
// definition for create and for both kernels) and the pinned-order arithmetic helpers.  The scalar controller of the iteration is nmpc_ipm.h;
// reciprocals, qdiv, LogSum, uniform_f64 and the reductions are nmpc_wave.h, which the LIDAR kernel includes as well.
// NOT shared, on purpose: each kernel's LDS layout sits next to it (ColLayout, LdsLayout; kernel 1's workspace is carved up by fill_params,
// HbmWs in nmpc_device.h naming its two structured arrays); kernel 1 keeps its own constraint arithmetic (slot_h, slot_jd, jxT_robot and its
// stage-0 pre-check in nmpc_kernels.hip), which rounds differently from the fma-pinned h_pair / h_obs below — unifying it would move kernel 1's
// results; init_barrier, merit, the stage-parallel phases and the sweeps belong to each kernel's data layout and stay there.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "nmpc_device.h"
#include "nmpc_ipm.h"
#include "nmpc_wave.h"

namespace nmpc {

template <int M_, int THB> struct G2 {
    static constexpr int NX = 3 * M_, NU = 2 * M_, NP = M_ * (M_ - 1) / 2, NZ = NX + NU, LD = NZ + 1;
    static constexpr int NXB = M_ * (2 + THB);
    static constexpr int NT = NZ * (NZ + 1) / 2 + NZ;   // upper triangle + rhs column
    // stage pack layout (doubles)
    static constexpr int PK_G = 0;                 // [NZ]  rhs gradient  (u part then x part)
    static constexpr int PK_HD = NZ;               // [NZ]  diagonal Hessian additions (without delta)
    static constexpr int PK_HXY = 2 * NZ;          // [M]   (x_i,y_i) entry of robot i's diagonal block
    static constexpr int PK_HVT = 2 * NZ + M_;     // [M]   (v_i,theta_i) cross term
    static constexpr int PK_E = 2 * NZ + 2 * M_;   // [3 NP] NEGATED pair blocks -E_ij
    static constexpr int PK_C = PK_E + 3 * (NP > 0 ? NP : 0);   // [NX]  defects c_k
    static constexpr int PK_CF = PK_C + NX;        // [NZ][3] coefficients of the <=3 terms of each row/column of [B A]
    static constexpr int PK_ZERO = PK_CF + 3 * NZ; // one zero entry (target of "no Hessian addition")
    static constexpr int PACK = ((PK_ZERO + 1 + 7) / 8) * 8;
    static constexpr int LDG = NZ + 1;             // row stride of G = P [B A | b-part]
    // element e of the row-major upper triangle (+ rhs column) lives in row row_of(e); thread tid owns e = tid + t*TPB, so
    // "slice" t holds rows slice_lo(t)..slice_hi(t): compile-time knowledge of which slices a pivot step touches
    static constexpr int row_of(int e) { int a = 0; while (e >= NZ - a + 1) { e -= NZ - a + 1; a++; } return a; }
    static constexpr int diag_e(int j) { int e = 0; for (int a = 0; a < j; a++) e += NZ - a + 1; return e; }   // flat index of element (j,j)
    static constexpr int slice_lo(int t, int tpb) { return row_of(t * tpb); }
    static constexpr int slice_hi(int t, int tpb) { return row_of((t * tpb + tpb - 1 < NT) ? (t * tpb + tpb - 1) : (NT - 1)); }
    // per stage: the NU pivot rows.  Element-per-lane kernel: [Uuu | Uux | rhs] at row stride LD, then the NU reciprocal pivots.
    // Column-per-lane kernel: the rows scaled by -1/pivot, [-Uuu/d (strictly upper part, else 0) | -Uux/d | -rhs/d | pad] at the
    // even row stride LDC (16-byte aligned rows: the forward sweep loads its row with dwordx4)
    static constexpr int LDC = (NZ + 3) & ~1;
    static constexpr int KTS = ((NU * LD + NU > NU * LDC ? NU * LD + NU : NU * LDC) + 7) / 8 * 8;
    // what the sweeps rely on: either kernel's rows fit the slot, and column NZ + 1 of a row of the column kernel — the padding slot its idle
    // lanes store to, also one slot ahead (the deferred store of row NU - 1) — lies inside the row
    static_assert(NU * LD + NU <= KTS && NU * LDC <= KTS && NZ + 1 < LDC, "a stage factor and its padding slots stay inside [KTS]");
};

// Where one instance of the two LDS-resident kernels keeps its arrays in the workspace, in doubles from the instance's base; every array
// starts on a 128-byte boundary.  Create copies the offsets into KParams (lds_workspace_fill) and the kernels read them from there —
// computing them in the kernel costs scalar registers the column kernel does not have; the sizes of a slot and of the two halves of the
// elastic block the kernels take from here.
template <int M_, int THB> struct WsLayout {
    using G = G2<M_, THB>;
    static constexpr int PACKS_BEYOND = 1;                     // packs behind the N stage packs: the terminal one ([2*NX] of it used)
    static constexpr int CKPT_PP = G::NX * G::NX + G::NX;      // the element-per-lane kernel saves [P | p] in a slot,
    static constexpr int CKPT_SLOT = (G::NX + 1) * 64;         // the column kernel its NX + 1 registers lane by lane: the slot's doubles
    static_assert(CKPT_PP <= CKPT_SLOT, "[P | p] of the element-per-lane kernel fits a checkpoint slot");
    static __host__ __device__ constexpr int ckpt_slots(int N) { return (N - 1) / NMPC_CKPT_EVERY + 1; }      // cost-to-go saved every NMPC_CKPT_EVERY stages of the backward sweep
    static __host__ __device__ constexpr int el_pair(int N1) { return N1 * G::NP; }                          // elastic block: t of the pair rows [N1][NP] (N1 = N + 1),
    static __host__ __device__ constexpr int el_obs(int N, int K) { return (N + 1) * M_ * K; }                // then of the obstacle rows [N1][M K]
    // [N + 1][G::PACK] stage packs (the column kernel's are shorter, GC) | [N][KTS] stage factors | [dual] the column kernel's slacks and duals
    // (ColLayout::dual) | [ckpt_slots][CKPT_SLOT] | [el_pair + el_obs] (elastic phase only)
    int64_t PACK, KT, DUAL, CKPT, ELAS, total;
    __host__ __device__ WsLayout(int N, int K, int dual)
    {
        int64_t o = 0;
        auto take = [&](int64_t n) { const int64_t at = o; o += (n + 15) / 16 * 16; return at; };
        PACK = take((int64_t)(N + PACKS_BEYOND) * G::PACK); KT = take((int64_t)N * G::KTS); DUAL = take(dual);
        CKPT = take((int64_t)ckpt_slots(N) * CKPT_SLOT); ELAS = take((int64_t)el_pair(N + 1) + el_obs(N, K));
        total = o;
    }
};

// ---- the obstacle field: component c (0 ox, 1 oy, 2 r) of obstacle o as the obstacle rows of stage k (evaluated at X_k) of one instance see
// it.  Every obstacle read of the solve and evaluation kernels goes through here; where the field comes from is a compile-time choice of the
// instantiation, never a run-time branch:
//   OS = 0  the handle's config field P.obs, a kernel argument shared by every instance and stage (nmpc_solve_batch and its kin);
//   OS = 1  the per-instance field of the *_obs entry points, P.ofield.ptr [B][S][K][3] in device memory: the instance's base is wave-uniform
//           (scalar registers), the element offset a 32-bit index (saddr addressing); the stage stride is 0 for a static field (S = 1).
template <int OS> struct ObsField {
    const KParams &P;
    const double *f;      // OS = 1: the instance's [S][K][3]
    __device__ __forceinline__ ObsField(const KParams &P_, size_t inst) : P(P_), f(nullptr)
    {
        if constexpr (OS != 0) f = P_.ofield.ptr + inst * (size_t)P_.ofield.istride;
    }
    __device__ __forceinline__ double operator()(int k, int o, int c) const
    {
        if constexpr (OS != 0)
            return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(f) + (size_t)((uint32_t)(k * P.ofield.sstride + 3 * o + c) * 8u));
        else
            return P.obs[3 * o + c];
    }
};

// ---- the pose reference of the cost: component c (0 .. NX-1) of the pose that the cost of stage k measures X_k against.  Every such read of
// the column kernel goes through here; where the row comes from is a compile-time choice of the instantiation, never a run-time branch:
//   TR = 0  the goal, the xs half of p, staged once as XS [NX] in LDS and the same for every stage (nmpc_solve_batch and its kin);
//   TR = 1  row k of the instance's reference R.ptr [B][S][NX] in device memory (the *_ref solve calls, track_col_kernel): wave-uniform base,
//           32-bit element offset (saddr addressing, as ObsField<1>); the stage stride is 0 for a single row (S = 1).  XS is never loaded.
template <int TR> struct PoseRows {
    const double *XS;     // TR = 0: [NX] in LDS
    const PoseRef &R;     // TR = 1: the kernel argument
    const double *f;      //         the instance's [S][NX]
    __device__ __forceinline__ PoseRows(const double *XS_, const PoseRef &R_, size_t inst) : XS(XS_), R(R_), f(nullptr)
    {
        if constexpr (TR != 0) f = R_.ptr + inst * (size_t)R_.istride;
    }
    __device__ __forceinline__ double operator()(int k, int c) const
    {
        if constexpr (TR != 0)
            return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(f) + (size_t)((uint32_t)(k * R.sstride + c) * 8u));
        else
            return XS[c];
    }
};

// ---- single evaluation points.  Constraint values, slack steps and defects are recomputed at several places of an
// iteration (Newton right-hand side, step-size rule, multiplier recursion, update).  With sigma = z/s up to 1e13 a
// last-bit difference between two sites (e.g. a differently contracted a*b+c) shows up as 1e-7 in the dual residual, so
// every site goes through these helpers, whose operation order is pinned with explicit fma().
// Their divisions go through qdiv (nmpc_wave.h) for the same reason.
__device__ __forceinline__ double h_pair(double ex, double ey, double dmin2) { return fma(ex, ex, ey * ey) - dmin2; }
__device__ __forceinline__ double ds_pair(double ex, double ey, double ddx, double ddy, double dmin2, double sv)
{
    return fma(2.0 * ex, ddx, (2.0 * ey) * ddy) + (h_pair(ex, ey, dmin2) - sv);
}
__device__ __forceinline__ double r_obs(double ex, double ey) { return sqrt(fma(ex, ex, ey * ey)); }
__device__ __forceinline__ double h_obs(double rr, double robdim, double orad, double margin) { return rr - robdim - orad - margin; }
__device__ __forceinline__ double ds_obs(double ex, double ey, double rr, double d0, double d1, double hv, double sv)
{
    return qdiv(fma(ex, d0, ey * d1), rr) + (hv - sv);
}
__device__ __forceinline__ double defect_xy(double xn, double x, double tu, double cs) { return xn - fma(tu, cs, x); }   // tu = T*v
__device__ __forceinline__ double defect_th(double xn, double x, double T, double w) { return xn - fma(T, w, x); }
__device__ __forceinline__ double ds_bound(double jd, double hv, double sv) { return jd + (hv - sv); }
__device__ __forceinline__ double dz_of(double mu, double sv, double zv, double ds) { return qdiv(fma(-zv, ds, fma(-sv, zv, mu)), sv); }

// ---- elastic phase (the second restart of last resort; derivation in oracle/nmpc_oracle.c): a pair / obstacle row h + t - s = 0, s, t >= 0,
// dual z in (0, rho).  jd = J dx of the row (ds_pair / ds_obs minus their (h - s) term).
__device__ __forceinline__ double jd_pair(double ex, double ey, double ddx, double ddy) { return fma(2.0 * ex, ddx, (2.0 * ey) * ddy); }
__device__ __forceinline__ double jd_obs(double ex, double ey, double rr, double d0, double d1) { return qdiv(fma(ex, d0, ey * d1), rr); }
__device__ __forceinline__ void el_sigma(double mu, double rho, double sv, double zv, double tv, double hv, double &sg, double &v)
{
    const double rz = rho - zv, D = qdiv(sv, zv) + qdiv(tv, rz), q = hv - qdiv(mu, zv) + qdiv(mu, rz);
    sg = qdiv(1.0, D); v = zv - q * sg;
}
__device__ __forceinline__ void el_step(double mu, double rho, double sv, double zv, double tv, double hv, double jd, double &ds, double &dz, double &dt)
{
    const double rz = rho - zv, D = qdiv(sv, zv) + qdiv(tv, rz), q = hv - qdiv(mu, zv) + qdiv(mu, rz);
    dz = -qdiv(jd + q, D);
    ds = qdiv(mu - sv * zv - sv * dz, zv);
    dt = qdiv(mu - tv * rz + tv * dz, rz);
}

// compile-time loop: f(std::integral_constant<int, I>) for I = B .. E-1 (indices usable in `if constexpr`)
template <int B, int E, class F> __device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// LDS access through a per-thread byte offset fixed at kernel start plus a compile-time constant: lowers to
// ds_read_b64 / ds_write_b64 with the constant in the instruction's offset field (no address arithmetic in the hot loops)
__device__ __forceinline__ double lds_ld(const double *sm, int byteoff, int cbytes)
{
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(sm) + byteoff + cbytes);
}
__device__ __forceinline__ void lds_st(double *sm, int byteoff, int cbytes, double v)
{
    *reinterpret_cast<double *>(reinterpret_cast<char *>(sm) + byteoff + cbytes) = v;
}

// LDS-only synchronisation of the threads of one instance.  __syncthreads() also drains vmcnt, i.e. it waits for every
// global load/store in flight — which would turn the stage-ahead prefetches of the sweeps into synchronous loads.  One
// wave executes its LDS instructions in order, so a single-wave instance only needs the LDS counter and a compiler fence;
// multi-wave instances add the hardware barrier.
template <int TPB> __device__ __forceinline__ void lds_sync()
{
    // release/acquire fences restricted to the LDS address space ("local"): s_waitcnt lgkmcnt(0) only, vmcnt untouched
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    if constexpr (TPB > 64) __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// reciprocal of a pivot: v_rcp_f64 seed + Newton steps.  NMPC_RCP_STEPS = 1 (round 4): the seed is good to about single precision, one step
// leaves <= 2.0e-15 relative (1.9e-15 measured, docs/WAVE_PRIMITIVES.md) — the factorisation of an interior-point step does not need more (iteration counts of the bench batches equal to
// 1e-5 relative, parity tests unchanged) and the two dependent multiply-adds it saves sit on the pivot chain of every stage: A/B in one
// session, six robots B=4096 +2.3 %, B=16384 +1.2 %.  2 = full fp64 accuracy (rounds 2-3; rcp2 of nmpc_wave.h, which the LIDAR kernel always takes).
#ifndef NMPC_RCP_STEPS
#define NMPC_RCP_STEPS 1
#endif
__device__ __forceinline__ double rcp_nr(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
#if NMPC_RCP_STEPS >= 2
    r = fma(fma(-d, r, 1.0), r, r);
#endif
    return r;
}

template <int M_> __device__ __forceinline__ int pidx(int a, int b) { return a * (2 * M_ - a - 1) / 2 + (b - a - 1); }

// flat index of the unordered pair {a, b}, a != b
template <int M_> __device__ __forceinline__ int pidx_any(int a, int b) { const int lo = a < b ? a : b, hi = a < b ? b : a; return pidx<M_>(lo, hi); }

// Inverse of pidx: pair (i < j) of flat index q (lexicographic order 12, 13, .., 1m, 23, .. of C6:288-306), without a loop.  The obvious
// `while (q >= M-1-i) { q -= M-1-i; i++; }` compiles to a DIVERGENT loop (11 instructions per trip, every lane waits for the lane with the
// largest i): ~60 issue slots per call, 25 calls per interior-point iteration of six robots.  Up to six robots (<= 15 pairs) i and j are
// 4-bit fields of two 64-bit literals; beyond, i counts the row starts c_r = r (2M-1-r)/2 that q has passed.
template <int M_> struct PairTab {
    static constexpr int NP = M_ * (M_ - 1) / 2;
    static constexpr unsigned long long tab(bool want_j)
    {
        unsigned long long t = 0;
        int q = 0;
        for (int i = 0; i < M_ && q < 16; i++)
            for (int j = i + 1; j < M_ && q < 16; j++, q++) t |= (unsigned long long)(want_j ? j : i) << (4 * q);
        return t;
    }
};
template <int M_> __host__ __device__ __forceinline__ constexpr void pair_of(int q, int &i, int &j)
{
    if constexpr (M_ * (M_ - 1) / 2 <= 16) {
        constexpr unsigned long long TI = PairTab<M_>::tab(false), TJ = PairTab<M_>::tab(true);
        const int sh = 4 * q;
        i = (int)((TI >> sh) & 15ull); j = (int)((TJ >> sh) & 15ull);
    } else {
        int r = 0;
#pragma unroll
        for (int s = 1; s < M_ - 1; s++) r += (q >= s * (2 * M_ - 1 - s) / 2) ? 1 : 0;
        i = r; j = q - r * (2 * M_ - 1 - r) / 2 + r + 1;
    }
}
// compile-time check of pair_of against the definition (the lexicographic enumeration) for every team size the kernels are instantiated for
template <int M_> constexpr bool pair_of_ok()
{
    int q = 0;
    for (int i = 0; i < M_; i++)
        for (int j = i + 1; j < M_; j++, q++) {
            int a = -1, b = -1;
            pair_of<M_>(q, a, b);
            if (a != i || b != j || a * (2 * M_ - a - 1) / 2 + (b - a - 1) != q) return false;
        }
    return q == M_ * (M_ - 1) / 2;
}
static_assert(pair_of_ok<1>() && pair_of_ok<2>() && pair_of_ok<3>() && pair_of_ok<4>() && pair_of_ok<5>() && pair_of_ok<6>() && pair_of_ok<7>() &&
              pair_of_ok<8>() && pair_of_ok<9>() && pair_of_ok<10>(), "pair_of is the inverse of pidx");

// ---- the simple bounds of the swarm NLP (C6:349-352); thb: the heading is bounded as well (kernel 1 passes P.thb, the others their THB)
__device__ __forceinline__ double lbu(const KParams &P, int c) { return (c & 1) ? -P.wmax : -P.vmax; }      // lower bound of control c (the upper one is its negative)
__device__ __forceinline__ int bst(int thb, int s) { return thb ? s : 3 * (s >> 1) + (s & 1); }             // bounded-state slot -> state index
__device__ __forceinline__ double bvl(const KParams &P, int thb, int s) { return (thb && (s % 3 == 2)) ? P.thmax : P.xymax; }
constexpr double NMPC_BOUND_PUSH = 1e-2;      // IPOPT bound_push = bound_frac
// push control c into the interior of its bounds (state component: push_state below)
__device__ __forceinline__ double push_control(const KParams &P, int c, double v)
{
    constexpr double bp = NMPC_BOUND_PUSH;
    double lo = lbu(P, c), hi = -lo, pu = fmin(bp * fmax(1.0, fabs(lo)), bp * (hi - lo));
    return fmin(fmax(v, lo + pu), hi - pu);
}
// ... as the LDS-resident kernels hold them: a reference and the flag, the shape of the closures this replaces.  lbu, bvl and push_control
// repeat the bodies above on purpose: forwarding to the free functions changes how the column kernel reaches the bound constants (scalar
// loads) and four of its symbols then gain scratch (docs/IPM_CONTROL.md).
struct Bounds {
    const KParams &P;
    const int thb;
    __device__ __forceinline__ double lbu(int c) const { return (c & 1) ? -P.wmax : -P.vmax; }
    __device__ __forceinline__ int bst(int s) const { return nmpc::bst(thb, s); }
    __device__ __forceinline__ double bvl(int s) const { return (thb && (s % 3 == 2)) ? P.thmax : P.xymax; }
    __device__ __forceinline__ double push_control(int c, double v) const
    {
        constexpr double bp = NMPC_BOUND_PUSH;
        double lo = lbu(c), hi = -lo, pu = fmin(bp * fmax(1.0, fabs(lo)), bp * (hi - lo));
        return fmin(fmax(v, lo + pu), hi - pu);
    }
};
// push state component c of a stage into the interior of its bounds.  Both bounds are read before the choice between them: written as
// (d == 2) ? P.thmax : P.xymax the choice becomes one between two addresses and the load a vector load from the parameter block.
__device__ __forceinline__ double push_state(const KParams &P, int thb, int c, double v)
{
    constexpr double bp = NMPC_BOUND_PUSH;
    const int d = c % 3;
    const double thmax = P.thmax, xymax = P.xymax;
    if (d < 2 || thb) {
        double b = (d == 2) ? thmax : xymax, px = fmin(bp * fmax(1.0, b), bp * 2.0 * b);
        v = fmin(fmax(v, -b + px), b - px);
    }
    return v;
}
// The primal point of a (re)start of the barrier iteration in the LDS-resident kernels: cold — the reference's cold start X_k = x0, U = 0
// (C6:398-400) — or the current point; either way pushed strictly inside the simple bounds (a control sitting on its bound would restart with
// a slack of ~1e-6 and a dual of mu / 1e-6), multipliers 0.  Slacks and duals follow in each kernel's init_barrier.
template <int M_, int THB, int TPB> __device__ __forceinline__ void restart_point(const KParams &P, const Bounds &bnd, bool cold, double *X, double *U, double *LAM)
{
    constexpr int NX = 3 * M_, NU = 2 * M_;
    const int tid = threadIdx.x, N = P.N, N1 = P.N + 1;
    if (cold) {
        for (int e = tid + NX; e < N1 * NX; e += TPB) X[e] = X[e % NX];
        for (int e = tid; e < N * NU; e += TPB) U[e] = 0.0;
        __syncthreads();
    }
    for (int e = tid + NX; e < N1 * NX; e += TPB) {
        X[e] = push_state(P, THB, e % NX, X[e]);
        LAM[e] = 0.0;
    }
    for (int e = tid; e < N * NU; e += TPB) U[e] = bnd.push_control(e % NU, U[e]);
    __syncthreads();
}
// what a solve reports per instance (one thread writes it): the infeasible-x0 exit and the normal exit of every swarm kernel
__device__ __forceinline__ void write_result(size_t inst, double obj, int status, int iters, double kkt, double *obj_out, int32_t *status_out, int32_t *iters_out,
                                             double *kkt_out)
{
    if (obj_out) obj_out[inst] = obj;
    if (status_out) status_out[inst] = status;
    if (iters_out) iters_out[inst] = iters;
    if (kkt_out) kkt_out[inst] = kkt;
}

#ifdef NMPC_PROFILE
#define PROF_T(i)                                                                                                                 \
    do {                                                                                                                          \
        long long _t = clock64();                                                                                                 \
        prof[i] += _t - tlast;                                                                                                    \
        tlast = _t;                                                                                                               \
    } while (0)
#else
#define PROF_T(i) do { } while (0)
#endif

}  // namespace nmpc
