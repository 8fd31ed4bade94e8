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
// iterations, from and to its state block, whose layout is the LDS image itself.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"

namespace lgs {
namespace {

// The value of lane l (wave-uniform l) in every lane.
__device__ inline double lll_bcast(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

__device__ inline bool lll_good(double x) { return x > 0.0 && x < INFINITY; }

struct LllLds {
    int64_t* b;
    int64_t* U;
    int64_t* G;
    double* mu;
    double* rdiag;
    int64_t* hdr;
};

__device__ inline LllLds lll_lds(int64_t* lds, int d) {
    const size_t n = (size_t)d * lll_ld(d);
    LllLds s;
    s.b = lds;
    s.U = lds + n;
    s.G = lds + 2 * n;
    s.mu = (double*)(lds + 3 * n);
    s.rdiag = s.mu + n;
    s.hdr = (int64_t*)(s.rdiag + kLllLanes);
    return s;
}

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
    int64_t* st = a.state + (size_t)q * words;
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
    int k = (int)s.hdr[0];
    int64_t iters = s.hdr[1], swaps = s.hdr[2], passes = s.hdr[3];
    int status = (int)s.hdr[4];
    double rd = s.rdiag[lane];  // r[lane][lane]
    const bool act = lane < d;
    int64_t budget = a.slice;
    while (status < 0) {
        if (k >= d) {
            status = 0;
            break;
        }
        if (iters == a.max_iters) {
            status = 1;
            break;
        }
        if (budget == 0) break;
        --budget;
        ++iters;
        double muk = 0.0;  // mu[k][lane]
        double rkk = 0.0;  // r[k][k]
        for (;;) {       // size-reduce b_k against b_{k-1} .. b_0
            ++passes;
            // chol(k), j < k: lane j owns r[k][j]; before step i lane i holds its final value
            const int row = lane < k ? lane : k - 1;
            const double* mrow = s.mu + row * ld;
            double sj = (double)s.G[k * ld + row];
            int i = 0;
            for (; i + 8 <= k; i += 8) {  // (eight LDS reads in flight; the order of the sum stays)
                double m[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) m[u] = mrow[i + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double rki = lll_bcast(sj, i + u);
                    const double t = sj - m[u] * rki;
                    sj = lane > i + u ? t : sj;
                }
            }
            for (; i < k; ++i) {
                const double rki = lll_bcast(sj, i);
                const double t = sj - mrow[i] * rki;
                sj = lane > i ? t : sj;
            }
            muk = lane < k ? sj / rd : 0.0;
            // j = k: its terms mu[k][i] r[k][i] are lane i's, subtracted in the order of i
            const double term = muk * sj;
            rkk = (double)s.G[k * ld + k];
            for (i = 0; i < k; ++i) rkk = rkk - lll_bcast(term, i);
            if (lane == k) rd = rkk;
            // b_k -= X b_j for j = k-1 .. 0 where |mu[k][j]| > eta; lane c owns coordinate c
            int64_t bk = act ? s.b[k * ld + lane] : 0;
            int64_t uk = act ? s.U[k * ld + lane] : 0;
            // (the next j is the highest lane below the last one whose coefficient exceeds eta:
            // a ballot finds it, and an update changes only the coefficients below it)
            bool applied = false;
            for (int jtop = k;;) {
                const unsigned long long exceed = __ballot(lane < jtop && fabs(muk) > a.eta);
                if (!exceed) break;
                const int j = 63 - __clzll((long long)exceed);
                jtop = j;
                const double m = lll_bcast(muk, j);
                const double X = rint(m);
                if (!(fabs(X) < kLllMaxX)) {
                    status = 2;
                    break;
                }
                const int64_t Xi = (int64_t)X;
                int64_t nb = 0, nu = 0;
                if (act) {
                    nb = bk - Xi * s.b[j * ld + lane];
                    nu = uk - Xi * s.U[j * ld + lane];
                }
                const bool over = nb >= kLllMaxB || nb <= -kLllMaxB || nu >= kLllMaxU || nu <= -kLllMaxU;
                if (__any(over)) {  // the state before this update is the result
                    status = 2;
                    break;
                }
                bk = nb;
                uk = nu;
                if (lane < j) muk = muk - X * s.mu[j * ld + lane];
                if (lane == j) muk = muk - X;
                applied = true;
            }
            if (act) {
                s.b[k * ld + lane] = bk;
                s.U[k * ld + lane] = uk;
            }
            if (lane < k) s.mu[k * ld + lane] = muk;
            __syncthreads();
            if (status >= 0 || !applied) break;
            if (act) {  // row and column k of G from b, exactly; lane j owns G[k][j]
                int64_t g = 0;
#pragma unroll 4
                for (int c = 0; c < d; ++c) g += s.b[k * ld + c] * s.b[lane * ld + c];
                s.G[k * ld + lane] = g;
                s.G[lane * ld + k] = g;
            }
            __syncthreads();
        }
        if (status >= 0) break;
        // Lovasz test
        if (!lll_good(rkk)) {
            status = 3;
            break;
        }
        const double m1 = lll_bcast(muk, k - 1);
        double t = m1 * m1;
        t = a.delta - t;
        t = t * lll_bcast(rd, k - 1);
        if (rkk >= t) {
            ++k;
            continue;
        }
        if (act) {  // swap b, U and the rows of G at k and k-1, then the columns of G
            const int p = k * ld + lane, o = (k - 1) * ld + lane;
            int64_t x = s.b[p];
            s.b[p] = s.b[o];
            s.b[o] = x;
            x = s.U[p];
            s.U[p] = s.U[o];
            s.U[o] = x;
            x = s.G[p];
            s.G[p] = s.G[o];
            s.G[o] = x;
        }
        __syncthreads();
        if (act) {
            const int p = lane * ld + k;
            const int64_t x = s.G[p];
            s.G[p] = s.G[p - 1];
            s.G[p - 1] = x;
        }
        __syncthreads();
        ++swaps;
        if (k == 1) {  // r[0][0] of the vector that moved to the front
            const double r00 = (double)s.G[0];
            if (lane == 0) rd = r00;
            if (!lll_good(r00)) {
                status = 3;
                break;
            }
        } else {
            --k;
        }
    }
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
