// lgs_kleinb.hip -- Klein draws and best-of-K decoding over a batch of bases (lgs_klein_bases,
// include/lgs.h): every basis brings its own targets and its own width, nothing
// is loaded into the context.  The factor R_p and the centres c'_{p,k} come from cvpb_qr_kernel
// (lgs_cvpb.hip), the QR(p) of lgs.h.
//
// kleinb_draw_kernel    blocks of kleinb_lanes(d) lanes, each block inside one basis: lane m of
//                       the basis is draw (k, j) = (m / K, m % K).  The block stages its basis's
//                       R, R_ii, s_i and the centres its lanes touch in LDS; the lane's
//                       coefficients live in LDS too, coordinate-major, as fp64.  The draw is
//                       klein_targets_exact_body<ZT, true> of lgs_kernels.hip, term for term.
// kleinb_select_kernel  one wave per problem (p, k): the smallest of its K distances, ties to
//                       the smallest j; the winner's row, its lattice point in the defined order.
//
// All fp64 arithmetic is unfused (the Makefile compiles with -ffp-contract=off); the division
// is IEEE-correct.  Nothing here depends on the block size: a lane reads only its basis's
// constants and its own column.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_device.h"
#include "lgs_kernels.h"

namespace lgs {
namespace {

constexpr int kSelectWaves = 4;  // problems per block of kleinb_select_kernel

// LDS (doubles): Rs d x d | rii d | sg d | cps d x nt, (i, kk) at [i * nt + kk] | zs d x L,
// (j, lane) at [j * L + lane].  Row i of Rs is read by every lane at the same address (a
// broadcast, so it needs no padding); a wave's reads of zs[j * L + ...] and of cps[i * nt + ...]
// are consecutive or repeated words.
__global__ __launch_bounds__(256) void kleinb_draw_kernel(const KleinbArgs a) {
    extern __shared__ double lds[];
    const int d = a.d, T = a.T, L = blockDim.x, tid = threadIdx.x;
    const int64_t K = a.K, TK = (int64_t)T * K;
    const int64_t nb = (TK + L - 1) / L;  // blocks of a basis
    const int64_t q = (int64_t)blockIdx.x / nb;
    const int64_t m0 = ((int64_t)blockIdx.x % nb) * L;
    const int nl = (int)(TK - m0 < L ? TK - m0 : L);  // the block's live lanes
    const int nt = kleinb_nt(T, K, L);
    const int64_t k0 = m0 / K;
    double* Rs = lds;
    double* rii = Rs + d * d;
    double* sg = rii + d;
    double* cps = sg + d;
    double* zs = cps + d * nt;
    const size_t row0 = ((size_t)q * TK + m0);  // the block's first row of ZW / DW
    if (a.qr_status[q] != 0) {  // a refused basis: zero rows, +inf (block-uniform)
        for (size_t e = tid; e < (size_t)nl * d; e += L) {
            if (a.zb == 8)
                ((int64_t*)a.ZW)[row0 * d + e] = 0;
            else
                ((int32_t*)a.ZW)[row0 * d + e] = 0;
        }
        if (tid < nl) a.DW[row0 + tid] = INFINITY;
        return;
    }
    const double* Rq = a.R + (size_t)q * d * d;
    for (int e = tid; e < d * d; e += L) Rs[e] = Rq[e];
    const double sigma = a.sigma[q];
    for (int i = tid; i < d; i += L) {
        // lgs_set_basis's rule (R_ii > 0 after the sign fix)
        const double r = Rq[(size_t)i * d + i];
        const double sref = sigma / r;
        double s = sref;
        if (sref < 1e-10)
            s = 0.0;  // rounded, not drawn
        else if (sref > 1e10)
            s = fmin(sref, 1e6);
        rii[i] = r;
        sg[i] = s;
    }
    const int ntb = (int)((T - k0) < nt ? (T - k0) : nt);  // staged targets that exist
    const double* cq = a.cprime + ((size_t)q * T + k0) * d;
    for (int e = tid; e < ntb * d; e += L) cps[(e % d) * nt + e / d] = cq[e];
    __syncthreads();
    const bool live = tid < nl;
    unsigned int flags = 0;
    if (live) {
        const int64_t m = m0 + tid;
        const int kk = (int)(m / K - k0);
        const uint64_t s = a.base + (uint64_t)q * (uint64_t)TK + (uint64_t)m;
        CoordStream rs;
        rs.init(a.seed, (uint32_t)(s >> 32), (uint32_t)s);
        double D = 0.0;
        for (int i = d - 1; i >= 0; --i) {
            const double* Ri = Rs + i * d;
            double cs = 0.0;
            for (int j = i + 1; j < d; ++j) cs = cs + Ri[j] * zs[j * L + tid];
            const double t = cps[i * nt + kk] - cs;
            const double mu = t / rii[i];
            const double si = sg[i];
            double zi = 0.0;
            if (!(fabs(mu) < 4503599627370496.0)) {  // not finite, or not below 2^52
                flags |= kFlagNonFinite;
            } else if (si == 0.0) {
                zi = rint(mu);
            } else {
                const SampleZOut o = sample_z(mu, si, a.precision, false, rs.u((uint32_t)(d - 1 - i)), false, a.etab);
                zi = (double)o.z;
            }
            zs[i * L + tid] = zi;
            const double qz = Ri[i] * zi;
            const double r = t - qz;
            D = D + r * r;
        }
        if (!isfinite(D)) flags |= kFlagNonFinite;
        a.DW[row0 + tid] = D;
    }
    __syncthreads();
    // the block's rows are contiguous in ZW: element e is coordinate e % d of lane e / d
    for (size_t e = tid; e < (size_t)nl * d; e += L) {
        const double zv = zs[(e % d) * L + e / d];
        if (a.zb == 8) {
            ((int64_t*)a.ZW)[row0 * d + e] = (int64_t)zv;
        } else {
            const bool fits = zv < 2147483648.0 && zv > -2147483648.0;
            if (!fits) flags |= kFlagOverflow;
            ((int32_t*)a.ZW)[row0 * d + e] = fits ? (int32_t)zv : 0;
        }
    }
    if (flags) atomicOr(a.flags, flags);
}

// Wave w of a block is problem pk = 4 blockIdx + w.  Lane l scans j = l, l + 64, ... in
// ascending order and keeps the first smallest; the wave's reduction orders (D, j) pairs.
__global__ __launch_bounds__(64 * kSelectWaves) void kleinb_select_kernel(const KleinbArgs a) {
    const int d = a.d, T = a.T, lane = threadIdx.x & 63;
    const int64_t K = a.K;
    const int64_t pk = (int64_t)blockIdx.x * kSelectWaves + (threadIdx.x >> 6);
    if (pk >= a.m * T) return;
    const int64_t q = pk / T;
    const bool bad = a.qr_status[q] != 0;
    const size_t row = (size_t)pk * d;
    double bD = INFINITY;
    int64_t bj = -1;
    if (!bad) {
        const double* Dk = a.DW + (size_t)pk * K;
        for (int64_t j = lane; j < K; j += 64) {
            const double D = Dk[j];
            if (bj < 0 || D < bD) {
                bD = D;
                bj = j;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const double oD = __shfl_xor(bD, o);
            const int64_t oj = __shfl_xor(bj, o);
            if (oj >= 0 && (bj < 0 || oD < bD || (oD == bD && oj < bj))) {
                bD = oD;
                bj = oj;
            }
        }
    }
    const size_t src = ((size_t)pk * K + (bad ? 0 : bj)) * d;
    if (lane < d) {
        if (a.zb == 8)
            ((int64_t*)a.z)[row + lane] = bad ? 0 : ((const int64_t*)a.ZW)[src + lane];
        else
            ((int32_t*)a.z)[row + lane] = bad ? 0 : ((const int32_t*)a.ZW)[src + lane];
        double acc = 0.0;
        if (!bad) {
            const double* B = a.bases + (size_t)q * d * d + (size_t)lane * d;
            for (int j = 0; j < d; ++j) {
                const double zj = a.zb == 8 ? (double)((const int64_t*)a.ZW)[src + j]
                                            : (double)((const int32_t*)a.ZW)[src + j];
                acc = acc + B[j] * zj;
            }
        }
        a.v[row + lane] = acc;
    }
    if (lane == 0) {
        a.best[pk] = bj;
        a.dist2[pk] = bD;
        a.status[pk] = bad ? 3 : 0;
    }
}

bool kleinb_args_ok(const KleinbArgs& a) {
    return a.d >= 2 && a.d <= kCvpMaxD && a.T >= 1 && a.T <= kKleinbMaxT && a.K >= 1 && a.m >= 1 &&
           a.m <= kKleinbSlots && (a.zb == 4 || a.zb == 8) && (int64_t)a.T * a.K <= kKleinbMaxDraws && a.qr_status &&
           a.ZW && a.DW && a.flags;
}

}  // namespace

namespace launch {

hipError_t kleinb_draw(const KleinbArgs& a, hipStream_t st) {
    if (!kleinb_args_ok(a) || a.precision < 1 || !a.sigma || !a.R || !a.cprime) return hipErrorInvalidValue;
    const int L = kleinb_lanes(a.d);
    const int64_t TK = (int64_t)a.T * a.K;
    const int64_t grid = a.m * ((TK + L - 1) / L);
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    const size_t lds = kleinb_lds_bytes(a.d, a.T, a.K);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kleinb_draw_kernel,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kleinb_draw_kernel, dim3((unsigned)grid), dim3(L), lds, st, a);
    return hipGetLastError();
}

hipError_t kleinb_select(const KleinbArgs& a, hipStream_t st) {
    if (!kleinb_args_ok(a) || !a.bases || !a.z || !a.v || !a.best || !a.dist2 || !a.status) return hipErrorInvalidValue;
    const int64_t grid = (a.m * a.T + kSelectWaves - 1) / kSelectWaves;
    hipLaunchKernelGGL(kleinb_select_kernel, dim3((unsigned)grid), dim3(64 * kSelectWaves), 0, st, a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
