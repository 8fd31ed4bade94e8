// lgs_lll_loop.h -- the LLL main loop on the LDS image of one basis, shared by lgs_lll.hip
// (lgs_lll_reduce) and lgs_bkz.hip (lgs_bkz_reduce, which enters it again after every
// insertion).  One wave per basis; see lgs_lll.hip for the layout and the ownership of lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"

namespace lgs {

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

// The registers of a basis in work: k, the counters, the status (-1 = running) and lane i's
// r[i][i].
struct LllRun {
    int k;
    int64_t iters, swaps, passes;
    int status;
    double rd;
};

// `while k < d` of lgs.h from the state in LDS and `w`, for at most `budget` iterations (counted
// down).  Returns with w.status 0 (k reached d), 1, 2 or 3, or with -1 when the budget ran out.
__device__ inline void lll_loop(const LllLds& s, const int d, const int lane, const double delta, const double eta,
                                const int64_t max_iters, int64_t& budget, LllRun& w) {
    const int ld = lll_ld(d);
    const bool act = lane < d;
    int k = w.k;
    int64_t iters = w.iters, swaps = w.swaps, passes = w.passes;
    int status = w.status;
    double rd = w.rd;
    while (status < 0) {
        if (k >= d) {
            status = 0;
            break;
        }
        if (iters == max_iters) {
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
                const unsigned long long exceed = __ballot(lane < jtop && fabs(muk) > eta);
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
        t = delta - t;
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
    w.k = k;
    w.iters = iters;
    w.swaps = swaps;
    w.passes = passes;
    w.status = status;
    w.rd = rd;
}

}  // namespace lgs
