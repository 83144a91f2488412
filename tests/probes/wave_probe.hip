// wave_probe.hip — applies the arithmetic and wave primitives the solve kernels share (csrc/nmpc_wave.h, the shared part of
// csrc/nmpc_solve_common.h, the controller csrc/nmpc_ipm.h) to input tables and writes the raw bits of what they return.  It includes the
// project's headers and defines none of the probed functions; it holds no reference value and judges nothing: tests/test_gpu_wave_probe.py
// writes the tables and compares the dump with tests/wave_probe_ref.py.  Built with the library's own code-generation flags
// (build.codegen_flags()), once as the library is built and once with -DNMPC_FAST_DIV=0 -DNMPC_RCP_STEPS=2.
//
//   wave_probe <tables.bin> <dump.bin>        exit status != 0 on any I/O or HIP error
//
// Both files: int64 number of sections, then per section four int64 (id, a, b, c) and its 8-byte words.  Input sections hold a * b * c doubles:
// element-wise groups a rows of b columns (c = 1), the reductions a cases of b terms per lane for c lanes (term-major: [case][term][lane]).
// The dump repeats (id, a, words per row or case, c) and holds a * words * (c lanes) words.  One launch per section; the reductions run as one
// workgroup of c threads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "nmpc_solve_common.h"
#include "ipm_cases.h"

using namespace nmpc;

enum { G_RCP = 1, G_QDIV = 2, G_LOGSUM = 3, G_REDUCE = 4, G_PAIR = 5, G_BOUND = 6, G_IPM = 7, G_ROWS = 8 };
enum { R_H_PAIR = 0, R_DS_PAIR, R_R_OBS, R_H_OBS, R_DS_OBS, R_DEFECT_XY, R_DEFECT_TH, R_DS_BOUND, R_DZ_OF, R_JD_PAIR, R_JD_OBS, R_EL_SIGMA, R_EL_STEP };

static int words_out(int id)
{
    switch (id) {
    case G_RCP: return 4;         // seed, rcp1, rcp2, rcp_nr
    case G_QDIV: return 2;        // seed of the denominator, qdiv
    case G_LOGSUM: return 5;      // per lane: wlogsum<c>, wave_logsum, and the lane's accumulator (m, e, lo) before the reduction
    case G_REDUCE: return 4;      // per lane: wsum<c>, wmax<c>, wmin<c>, wave_min
    case G_PAIR: return 4;        // pair_of -> (i, j), pidx, pidx_any
    case G_BOUND: return 8;
    case G_IPM: return ipm_cases::OUT;
    case G_ROWS: return 3;
    }
    return 0;
}

__device__ __forceinline__ void put(uint64_t *o, double v) { *o = (uint64_t)__double_as_longlong(v); }

__global__ void rcp_kernel(const double *in, uint64_t *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double d = in[i];
    put(out + 4 * i, __builtin_amdgcn_rcp(d)); put(out + 4 * i + 1, rcp1(d)); put(out + 4 * i + 2, rcp2(d)); put(out + 4 * i + 3, rcp_nr(d));
}
__global__ void qdiv_kernel(const double *in, uint64_t *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    put(out + 2 * i, __builtin_amdgcn_rcp(in[2 * i + 1])); put(out + 2 * i + 1, qdiv(in[2 * i], in[2 * i + 1]));
}
template <int TPB> __global__ void __launch_bounds__(TPB) logsum_kernel(const double *in, uint64_t *out, int cases, int terms)
{
    __shared__ double red[TPB / 64];
    const int tid = threadIdx.x;
    for (int c = 0; c < cases; c++) {
        LogSum a;
        for (int t = 0; t < terms; t++) a.add(in[((size_t)c * terms + t) * TPB + tid]);
        uint64_t *o = out + (size_t)c * 5 * TPB;
        put(o + 2 * TPB + tid, a.m); put(o + 3 * TPB + tid, (double)a.e); put(o + 4 * TPB + tid, a.lo);
        put(o + tid, wlogsum<TPB>(a, red));
        __syncthreads();      // red is written again by the next case
        put(o + TPB + tid, wave_logsum(a));
    }
}
template <int TPB> __global__ void __launch_bounds__(TPB) reduce_kernel(const double *in, uint64_t *out, int cases)
{
    __shared__ double red[TPB / 64];
    const int tid = threadIdx.x;
    for (int c = 0; c < cases; c++) {
        const double v = in[(size_t)c * TPB + tid];
        uint64_t *o = out + (size_t)c * 4 * TPB;
        put(o + tid, wsum<TPB>(v, red)); __syncthreads();
        put(o + TPB + tid, wmax<TPB>(v, red)); __syncthreads();
        put(o + 2 * TPB + tid, wmin<TPB>(v, red)); __syncthreads();
        put(o + 3 * TPB + tid, wave_min(v));
    }
}
template <int M_> __device__ void pair_row(int q, int a, int b, uint64_t *o)
{
    int i = -1, j = -1;
    pair_of<M_>(q, i, j);
    put(o, (double)i); put(o + 1, (double)j); put(o + 2, (double)pidx<M_>(a, b)); put(o + 3, (double)pidx_any<M_>(a, b));
}
__global__ void pair_kernel(const double *in, uint64_t *out, int n)      // row: (M, q, a, b)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int m = (int)in[4 * r], q = (int)in[4 * r + 1], a = (int)in[4 * r + 2], b = (int)in[4 * r + 3];
    uint64_t *o = out + 4 * r;
    for (int k = 0; k < 4; k++) put(o + k, -1.0);      // a team size with no instantiation stays recognisable
    static_for<1, 11>([&](auto M) { if (m == M.value) pair_row<M.value>(q, a, b, o); });
}
__global__ void bound_kernel(const double *in, uint64_t *out, int n)      // row: (thb, c, v, vmax, wmax, xymax, thmax, -)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double *a = in + 8 * r;
    KParams P{};
    const int thb = (int)a[0], c = (int)a[1];
    const double v = a[2];
    P.vmax = a[3]; P.wmax = a[4]; P.xymax = a[5]; P.thmax = a[6];
    const Bounds bnd{P, thb};
    uint64_t *o = out + 8 * r;
    put(o, lbu(P, c)); put(o + 1, (double)bst(thb, c)); put(o + 2, bvl(P, thb, c)); put(o + 3, push_control(P, c, v)); put(o + 4, push_state(P, thb, c, v));
    put(o + 5, bnd.lbu(c)); put(o + 6, bnd.bvl(c)); put(o + 7, bnd.push_control(c, v));      // the copies the LDS-resident kernels hold
}
__global__ void ipm_kernel(const double *in, uint64_t *out, int n)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double o[ipm_cases::OUT];
    ipm_cases::apply(in + (size_t)ipm_cases::IN * r, o);
    for (int k = 0; k < ipm_cases::OUT; k++) put(out + (size_t)ipm_cases::OUT * r + k, o[k]);
}
__global__ void rows_kernel(const double *in, uint64_t *out, int n)      // row: (helper, up to seven arguments)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const double *a = in + 8 * r + 1;
    double o0 = 0.0, o1 = 0.0, o2 = 0.0;
    switch ((int)in[8 * r]) {
    case R_H_PAIR: o0 = h_pair(a[0], a[1], a[2]); break;
    case R_DS_PAIR: o0 = ds_pair(a[0], a[1], a[2], a[3], a[4], a[5]); break;
    case R_R_OBS: o0 = r_obs(a[0], a[1]); break;
    case R_H_OBS: o0 = h_obs(a[0], a[1], a[2], a[3]); break;
    case R_DS_OBS: o0 = ds_obs(a[0], a[1], a[2], a[3], a[4], a[5], a[6]); break;
    case R_DEFECT_XY: o0 = defect_xy(a[0], a[1], a[2], a[3]); break;
    case R_DEFECT_TH: o0 = defect_th(a[0], a[1], a[2], a[3]); break;
    case R_DS_BOUND: o0 = ds_bound(a[0], a[1], a[2]); break;
    case R_DZ_OF: o0 = dz_of(a[0], a[1], a[2], a[3]); break;
    case R_JD_PAIR: o0 = jd_pair(a[0], a[1], a[2], a[3]); break;
    case R_JD_OBS: o0 = jd_obs(a[0], a[1], a[2], a[3], a[4]); break;
    case R_EL_SIGMA: el_sigma(a[0], a[1], a[2], a[3], a[4], a[5], o0, o1); break;
    case R_EL_STEP: el_step(a[0], a[1], a[2], a[3], a[4], a[5], a[6], o0, o1, o2); break;
    default: break;
    }
    put(out + 3 * r, o0); put(out + 3 * r + 1, o1); put(out + 3 * r + 2, o2);
}

#define HIP_OK(x)                                                                                       \
    do {                                                                                                \
        const hipError_t e_ = (x);                                                                      \
        if (e_ != hipSuccess) {                                                                         \
            fprintf(stderr, "wave_probe: %s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

static int launch(int id, int a, int b, int c, const double *din, uint64_t *dout)
{
    const dim3 grid((unsigned)((a + 255) / 256)), blk(256);
    switch (id) {
    case G_RCP: if (b != 1 || c != 1) return 2; hipLaunchKernelGGL(rcp_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_QDIV: if (b != 2 || c != 1) return 2; hipLaunchKernelGGL(qdiv_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_PAIR: if (b != 4 || c != 1) return 2; hipLaunchKernelGGL(pair_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_BOUND: if (b != 8 || c != 1) return 2; hipLaunchKernelGGL(bound_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_IPM: if (b != ipm_cases::IN || c != 1) return 2; hipLaunchKernelGGL(ipm_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_ROWS: if (b != 8 || c != 1) return 2; hipLaunchKernelGGL(rows_kernel, grid, blk, 0, 0, din, dout, a); break;
    case G_LOGSUM:
        if (c == 64) hipLaunchKernelGGL(logsum_kernel<64>, dim3(1), dim3(64), 0, 0, din, dout, a, b);
        else if (c == 128) hipLaunchKernelGGL(logsum_kernel<128>, dim3(1), dim3(128), 0, 0, din, dout, a, b);
        else if (c == 256) hipLaunchKernelGGL(logsum_kernel<256>, dim3(1), dim3(256), 0, 0, din, dout, a, b);
        else return 2;
        break;
    case G_REDUCE:
        if (b != 1) return 2;
        if (c == 64) hipLaunchKernelGGL(reduce_kernel<64>, dim3(1), dim3(64), 0, 0, din, dout, a);
        else if (c == 128) hipLaunchKernelGGL(reduce_kernel<128>, dim3(1), dim3(128), 0, 0, din, dout, a);
        else if (c == 256) hipLaunchKernelGGL(reduce_kernel<256>, dim3(1), dim3(256), 0, 0, din, dout, a);
        else return 2;
        break;
    default: return 2;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: wave_probe <tables.bin> <dump.bin>\n"); return 2; }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi) { perror(argv[1]); return 2; }
    FILE *fo = fopen(argv[2], "wb");
    if (!fo) { perror(argv[2]); return 2; }
    int64_t nsec = 0;
    if (fread(&nsec, 8, 1, fi) != 1 || nsec < 0 || nsec > 4096) { fprintf(stderr, "wave_probe: bad table header\n"); return 2; }
    fwrite(&nsec, 8, 1, fo);
    for (int64_t s = 0; s < nsec; s++) {
        int64_t h[4];
        if (fread(h, 8, 4, fi) != 4) { fprintf(stderr, "wave_probe: truncated section header\n"); return 2; }
        const int64_t id = h[0], a = h[1], b = h[2], c = h[3];
        const int w = words_out((int)id);
        if (w == 0 || a < 1 || b < 1 || c < 1 || a > (1 << 22) || b > (1 << 16) || c > 256 || a * b * c > (1ll << 24)) {
            fprintf(stderr, "wave_probe: section %lld: bad shape (%lld, %lld, %lld, %lld)\n", (long long)s, (long long)id, (long long)a, (long long)b, (long long)c);
            return 2;
        }
        const bool red = id == G_LOGSUM || id == G_REDUCE;
        const size_t nin = (size_t)(a * b * c), nout = (size_t)a * w * (red ? (size_t)c : 1);
        std::vector<double> in(nin);
        std::vector<uint64_t> out(nout);
        if (fread(in.data(), 8, nin, fi) != nin) { fprintf(stderr, "wave_probe: truncated section %lld\n", (long long)s); return 2; }
        double *din = nullptr;
        uint64_t *dout = nullptr;
        HIP_OK(hipMalloc(&din, nin * 8));
        HIP_OK(hipMalloc(&dout, nout * 8));
        HIP_OK(hipMemcpy(din, in.data(), nin * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(dout, 0xff, nout * 8));
        if (launch((int)id, (int)a, (int)b, (int)c, din, dout)) { fprintf(stderr, "wave_probe: section %lld: no kernel for (%lld, %lld, %lld)\n", (long long)s, (long long)id, (long long)b, (long long)c); return 2; }
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), dout, nout * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipFree(din));
        HIP_OK(hipFree(dout));
        const int64_t ho[4] = {id, a, (int64_t)w, red ? c : 1};
        fwrite(ho, 8, 4, fo);
        if (fwrite(out.data(), 8, nout, fo) != nout) { fprintf(stderr, "wave_probe: short write\n"); return 2; }
    }
    fclose(fi);
    if (fclose(fo) != 0) { perror(argv[2]); return 2; }
    return 0;
}
