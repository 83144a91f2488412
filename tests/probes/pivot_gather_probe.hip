// One wavefront: the pivot row of a row-paired register replicated by lane swaps and by lane gathers (csrc/nmpc_solve_col.hip, step 5 of
// the row-paired stage; docs/PIVOT_GATHER.md), on registers of distinct lane tags, for a pivot row in the lower (hj = 0) and in the upper
// half (hj = 1).  One launch, 64 threads.      pivot_gather_probe <dump>
// dump: float64 [PATTERNS][2 (hj)][6][64]: the register, own by swaps, ur by swaps, the register as the swaps leave it, own by gathers,
// ur by gathers.  tests/test_gpu_pivot_gather.py compares the two forms with one another and with tools/rp_emu.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

constexpr int PATTERNS = 2, OUT = 6;

// the three primitives as the column kernel writes them
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void swap16(double &a, double &b)      // odd rows (of 16 lanes) of a <-> even rows of b
{
    u32x2 lo = __builtin_amdgcn_permlane16_swap(__double2loint(a), __double2loint(b), false, false);
    u32x2 hi = __builtin_amdgcn_permlane16_swap(__double2hiint(a), __double2hiint(b), false, false);
    a = __hiloint2double(hi.x, lo.x); b = __hiloint2double(hi.y, lo.y);
}
__device__ __forceinline__ void swap32(double &a, double &b)      // upper 32 lanes of a <-> lower 32 lanes of b
{
    u32x2 lo = __builtin_amdgcn_permlane32_swap(__double2loint(a), __double2loint(b), false, false);
    u32x2 hi = __builtin_amdgcn_permlane32_swap(__double2hiint(a), __double2hiint(b), false, false);
    a = __hiloint2double(hi.x, lo.x); b = __hiloint2double(hi.y, lo.y);
}
__device__ __forceinline__ double lane_gather(int src4, double v)     // v of lane src4 / 4
{
    return __hiloint2double(__builtin_amdgcn_ds_bpermute(src4, __double2hiint(v)), __builtin_amdgcn_ds_bpermute(src4, __double2loint(v)));
}

// lane tag: distinct in both 32-bit words of the double, exactly representable
__host__ __device__ inline double tag(int pattern, int lane) { return 1000.0 * (pattern + 1) + lane + (lane + 1) * 0x1p-40; }

template <int HJ> __device__ void both_forms(double reg, double *out, int tid, int gown, int gur)
{
    double own = reg, left = reg;
    if constexpr (HJ == 0) swap32(own, left); else swap32(left, own);
    double ur = own, ub = own;
    swap16(ur, ub);
    swap32(ur, ub);
    const double own_g = lane_gather(gown + 128 * HJ, reg), ur_g = lane_gather(gur + 128 * HJ, reg);
    out[0 * 64 + tid] = reg; out[1 * 64 + tid] = own; out[2 * 64 + tid] = ur; out[3 * 64 + tid] = left;
    out[4 * 64 + tid] = own_g; out[5 * 64 + tid] = ur_g;
}

__global__ void __launch_bounds__(64) probe(double *out)
{
    const int tid = threadIdx.x;
    const int gown = 4 * (tid & 31), gur = 4 * (16 * (tid >> 5) + (tid & 15));
    for (int p = 0; p < PATTERNS; p++) {
        both_forms<0>(tag(p, tid), out + (size_t)(2 * p + 0) * OUT * 64, tid, gown, gur);
        both_forms<1>(tag(p, tid), out + (size_t)(2 * p + 1) * OUT * 64, tid, gown, gur);
    }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <dump>\n", argv[0]); return 1; }
    const size_t n = (size_t)PATTERNS * 2 * OUT * 64;
    double *d = nullptr;
    CHECK(hipMalloc(&d, n * sizeof(double)));
    CHECK(hipMemset(d, 0xff, n * sizeof(double)));
    probe<<<1, 64>>>(d);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    std::vector<double> h(n);
    CHECK(hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
    CHECK(hipFree(d));
    FILE *f = fopen(argv[1], "wb");
    if (!f || fwrite(h.data(), sizeof(double), n, f) != n || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", argv[1]); return 1; }
    return 0;
}
