// lgs_lll.hip -- batched LLL basis reduction (lgs_lll_reduce, include/lgs.h).
//
// One basis per block of one wave.  The integer state (the vectors b, the transform U, the
// exact Gram matrix G) and the fp64 coefficients mu live in LDS for the whole launch, rows
// padded to an odd pitch, so that the two sweeps of the algorithm are both conflict-free: a
// lane owns a coordinate c for the vector updates (b[k][c] -= X b[j][c]: row reads), and owns
// an index j for the Gram row and for the Cholesky recurrence (b[j][c], mu[j][i]: column
// reads).  r[k][.] of the row in work is one register per lane -- lane j owns r[k][j] and the
// recurrence runs as a wavefront over i, r[k][i] broadcast from lane i once it is final -- and
// only the diagonal r[i][i] is kept (lane i's register, LDS between launches).
//
// The arithmetic is the operational definition of lgs.h: the integer sums are exact in any
// order, every fp64 value is produced by the same sequence of single operations (the Makefile
// compiles with -ffp-contract=off), and all control flow is wave-uniform, decided on broadcast
// values.  No launch is unbounded: a launch advances a basis by at most `slice` main-loop
// iterations, from and to its state block, whose layout is the LDS image itself.  The main loop
// is lll_loop of lgs_lll_loop.h, which lgs_bkz.hip enters too.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"
#include "lgs_lll_loop.h"

namespace lgs {
namespace {

// The state blocks of the chunk from the caller's bases: b (range-checked), U = I, the whole
// Gram matrix, mu = 0, chol(0) -- r[0][0] = (double)G[0][0] -- and k = 1.
__global__ __launch_bounds__(kLllLanes) void lll_init_kernel(const LllArgs a) {
    extern __shared__ int64_t lds[];
    const int d = a.d, ld = lll_ld(d), lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const size_t words = lll_state_words(d);
    const LllLds s = lll_lds(lds, d);
    for (size_t w = lane; w < words; w += kLllLanes) lds[w] = 0;
    __syncthreads();
    const int64_t* in = a.basis + (size_t)q * d * d;
    bool range = false;
    if (lane < d) {
        for (int c = 0; c < d; ++c) {
            int64_t v = in[(size_t)c * d + lane];
            if (v >= kLllMaxB || v <= -kLllMaxB) {
                range = true;
                v = 0;
            }
            s.b[lane * ld + c] = v;
        }
        s.U[lane * ld + lane] = 1;
    }
    if (range) atomicOr(a.flags, kLllFlagRange);
    __syncthreads();
    if (lane < d)
        for (int i = 0; i < d; ++i) {
            int64_t g = 0;
            for (int c = 0; c < d; ++c) g += s.b[i * ld + c] * s.b[lane * ld + c];
            s.G[i * ld + lane] = g;
        }
    __syncthreads();
    if (lane == 0) {
        const double r00 = (double)s.G[0];
        s.rdiag[0] = r00;
        s.hdr[0] = 1;
        s.hdr[4] = lll_good(r00) ? -1 : 3;
    }
    __syncthreads();
    // (lgs_bkz_reduce's state blocks are longer: the image, then its own words, zeroed by the host)
    int64_t* st = a.state + (size_t)q * (a.state_words ? a.state_words : words);
    for (size_t w = lane; w < words; w += kLllLanes) st[w] = lds[w];
}

__global__ __launch_bounds__(kLllLanes) void lll_reduce_kernel(const LllArgs a) {
    extern __shared__ int64_t lds[];
    const int d = a.d, ld = lll_ld(d), lane = threadIdx.x;
    const int64_t q = a.live_in ? a.live_in[blockIdx.x] : (int64_t)blockIdx.x;
    const size_t words = lll_state_words(d);
    const LllLds s = lll_lds(lds, d);
    int64_t* st = a.state + (size_t)q * words;
    for (size_t w = lane; w < words; w += kLllLanes) lds[w] = st[w];
    __syncthreads();
    LllRun w;
    w.k = (int)s.hdr[0];
    w.iters = s.hdr[1];
    w.swaps = s.hdr[2];
    w.passes = s.hdr[3];
    w.status = (int)s.hdr[4];
    w.rd = s.rdiag[lane];  // r[lane][lane]
    const bool act = lane < d;
    int64_t budget = a.slice;
    lll_loop(s, d, lane, a.delta, a.eta, a.max_iters, budget, w);
    const int k = w.k, status = w.status;
    const int64_t iters = w.iters, swaps = w.swaps, passes = w.passes;
    const double rd = w.rd;
    __syncthreads();
    if (status < 0) {  // suspended: the state back to its block, the basis onto the live list
        s.rdiag[lane] = rd;
        if (lane == 0) {
            s.hdr[0] = k;
            s.hdr[1] = iters;
            s.hdr[2] = swaps;
            s.hdr[3] = passes;
            s.hdr[4] = status;
            const unsigned long long at = atomicAdd(a.ctl, 1ull);
            if (at < (unsigned long long)a.nlive) a.live_out[at] = (int32_t)q;
        }
        __syncthreads();
        for (size_t w = lane; w < words; w += kLllLanes) st[w] = lds[w];
        return;
    }
    // stopped: the outputs in the caller's layout (vector i in column i); lane i reads column c
    // of its LDS row and the wave writes a row of the output
    int64_t* bo = a.basis_out + (size_t)q * d * d;
    int64_t* uo = a.U_out + (size_t)q * d * d;
    if (act) {
        for (int c = 0; c < d; ++c) {
            bo[(size_t)c * d + lane] = s.b[lane * ld + c];
            uo[(size_t)c * d + lane] = s.U[lane * ld + c];
        }
        if (a.gs_norm2) a.gs_norm2[(size_t)q * d + lane] = rd;
    }
    if (lane == 0) {
        if (a.swaps) a.swaps[q] = swaps;
        if (a.iters) a.iters[q] = iters;
        if (a.passes) a.passes[q] = passes;
        if (a.status) a.status[q] = status;
    }
}

hipError_t lll_check(const LllArgs& a) {
    if (a.d < 2 || a.d > kLllMaxD || a.m < 1 || !a.state || !a.flags) return hipErrorInvalidValue;
    return hipSuccess;
}

}  // namespace

namespace launch {

hipError_t lll_init(const LllArgs& a, hipStream_t st) {
    hipError_t e = lll_check(a);
    if (e != hipSuccess) return e;
    if (!a.basis) return hipErrorInvalidValue;
    const size_t lds = lll_lds_bytes(a.d);
    if (lds > 48 * 1024) {
        e = hipFuncSetAttribute((const void*)lll_init_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lll_init_kernel, dim3((unsigned)a.m), dim3(kLllLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t lll_reduce(const LllArgs& a, hipStream_t st) {
    if (a.nlive <= 0) return hipSuccess;
    hipError_t e = lll_check(a);
    if (e != hipSuccess) return e;
    if (a.nlive > a.m || !a.live_out || !a.ctl || !a.basis_out || !a.U_out || a.slice < 1 || a.max_iters < 1)
        return hipErrorInvalidValue;
    const size_t lds = lll_lds_bytes(a.d);
    if (lds > 48 * 1024) {
        e = hipFuncSetAttribute((const void*)lll_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(lll_reduce_kernel, dim3((unsigned)a.nlive), dim3(kLllLanes), lds, st, a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
