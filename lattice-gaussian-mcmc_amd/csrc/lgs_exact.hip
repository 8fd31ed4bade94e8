// lgs_exact.hip -- the exact sampler's table and draws (lgs_exact_table, lgs_exact_sample,
// include/lgs.h).
//
// The table is the listed ball of every target (lgs_ball_points' rows) with a weight and a
// running sum per row.  The running sum is the blocked one of lgs.h: sequential inside a
// block of kExactBlock rows and over a target's block totals, parallel over the blocks, so
// that NumPy reproduces every bit.  A draw is one Philox uniform, one multiply and a binary
// search of the target's S.  fp64, unfused (the Makefile compiles with -ffp-contract=off).
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"

namespace lgs {
namespace {

constexpr uint32_t kTagExact = 2;  // (0: the coordinate draws, 1: the accept draw)

// The uniform of a draw: Philox-4x32-10 with counter (0, step, chain, kTagExact) under the
// seed, words 0 and 1 as NumPy's 53-bit double -- lgs_device.h's generator in plain C++ (that
// header belongs to lgs_kernels.hip: it defines the Klein kernels' constant tables).
__device__ inline double exact_uniform(uint64_t seed, uint32_t step, uint32_t chain) {
    uint32_t c0 = 0u, c1 = step, c2 = chain, c3 = kTagExact;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

// The target that owns block g: the largest t with boff[t] <= g (boff[0] = 0, boff[n] > g;
// targets without rows own no block and are never found).
__device__ inline int64_t exact_owner(const int64_t* __restrict__ boff, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;  // boff[lo] <= g < boff[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (boff[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// One workgroup per block: the weights in parallel, then lane 0 adds them in row order.
__global__ __launch_bounds__(kExactBlock) void exact_weight_kernel(const ExactTable t, const double* shift,
                                                                   double two_s2) {
    __shared__ double w_s[kExactBlock];
    const int64_t g = blockIdx.x;
    const int64_t k = exact_owner(t.boff, t.n, g);
    const int64_t row0 = t.off[k] + (g - t.boff[k]) * kExactBlock;
    const int64_t left = t.off[k + 1] - row0;
    const int cnt = left < kExactBlock ? (int)left : kExactBlock;
    const int i = threadIdx.x;
    if (i < cnt) {
        const double sh = shift ? shift[k] : 0.0;
        const double w = exp((sh - t.D[row0 + i]) / two_s2);
        t.W[row0 + i] = w;
        w_s[i] = w;
    }
    __syncthreads();
    if (i == 0) {
        double run = 0.0;
        for (int r = 0; r < cnt; ++r) {
            run = run + w_s[r];
            w_s[r] = run;
        }
        t.btot[g] = run;
    }
    __syncthreads();
    if (i < cnt) t.S[row0 + i] = w_s[i];
}

// One lane per target: P_b of its blocks in order, and M.
__global__ __launch_bounds__(256) void exact_prefix_kernel(const ExactTable t) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= t.n) return;
    double p = 0.0;
    for (int64_t g = t.boff[k]; g < t.boff[k + 1]; ++g) {
        t.bpre[g] = p;
        p = p + t.btot[g];
    }
    t.mass[k] = p;
}

__global__ __launch_bounds__(kExactBlock) void exact_cum_kernel(const ExactTable t) {
    const int64_t g = blockIdx.x;
    const int64_t k = exact_owner(t.boff, t.n, g);
    const int64_t row = t.off[k] + (g - t.boff[k]) * kExactBlock + threadIdx.x;
    if (row < t.off[k + 1]) t.S[row] = t.bpre[g] + t.S[row];
}

// One lane per draw.  The selected row is copied into the chunk's coordinate-major store
// (adjacent lanes write adjacent elements; a lane reads its own row front to back), from
// where the caller's rows and B z are formed as for every other entry point.
template <typename TT, typename OT>
__global__ __launch_bounds__(256) void exact_draw_kernel(const ExactDrawArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    const uint64_t J = (uint64_t)(a.j0 + j);
    const int64_t t = (int64_t)(J / (uint64_t)a.K);
    const uint64_t s = a.first + J;
    const double tau = exact_uniform(a.seed, (uint32_t)(s >> 32), (uint32_t)s) * a.mass[t];
    const int64_t first = a.off[t], end = a.off[t + 1];
    int64_t lo = first, hi = end;  // the smallest row with S > tau lies in [lo, hi]
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.S[mid] > tau)
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo >= end) lo = end - 1;
    if (a.index) a.index[j] = lo;
    if (a.dist2) a.dist2[j] = a.D[lo];
    const TT* row = (const TT*)a.Z + (size_t)lo * a.d;
    OT* W = (OT*)a.W + j;
    bool over = false;
    for (int k = 0; k < a.d; ++k) {
        const int64_t v = (int64_t)row[k];
        if (sizeof(OT) == 4 && sizeof(TT) == 8 && (v >= (1ll << 31) || v <= -(1ll << 31))) over = true;
        W[(size_t)k * a.ldw] = (OT)v;
    }
    if (over) atomicOr(a.flags, kFlagOverflow);
}

}  // namespace

namespace launch {

hipError_t exact_scan(const ExactTable& t, const double* shift, double two_s2, hipStream_t st) {
    if (t.n <= 0 || t.nblocks <= 0) return hipSuccess;
    if (t.nblocks > 0x7fffffffll || !t.off || !t.boff || !t.D || !t.W || !t.S || !t.btot || !t.bpre || !t.mass)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(exact_weight_kernel, dim3((unsigned)t.nblocks), dim3(kExactBlock), 0, st, t, shift, two_s2);
    hipLaunchKernelGGL(exact_prefix_kernel, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, st, t);
    hipLaunchKernelGGL(exact_cum_kernel, dim3((unsigned)t.nblocks), dim3(kExactBlock), 0, st, t);
    return hipGetLastError();
}

hipError_t exact_draw(const ExactDrawArgs& a, int tb, int ob, hipStream_t st) {
    if (a.m <= 0) return hipSuccess;
    if (a.d < 1 || a.K < 1 || a.m > a.ldw || !a.off || !a.S || !a.D || !a.mass || !a.Z || !a.W ||
        (tb != 4 && tb != 8) || (ob != 4 && ob != 8))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.m + 255) / 256));
    if (tb == 4 && ob == 4)
        hipLaunchKernelGGL((exact_draw_kernel<int32_t, int32_t>), grid, dim3(256), 0, st, a);
    else if (tb == 4)
        hipLaunchKernelGGL((exact_draw_kernel<int32_t, int64_t>), grid, dim3(256), 0, st, a);
    else if (ob == 4)
        hipLaunchKernelGGL((exact_draw_kernel<int64_t, int32_t>), grid, dim3(256), 0, st, a);
    else
        hipLaunchKernelGGL((exact_draw_kernel<int64_t, int64_t>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
