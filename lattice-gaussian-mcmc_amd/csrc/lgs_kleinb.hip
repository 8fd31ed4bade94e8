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
// IMHK chains over the same batch (lgs_imhk_bases):
// kleinb_draw_wl_kernel the draw kernel on the counters (chain, step), every draw's Wang-Ling
//                       log weight where the distance was.
// imhkb_scan_kernel     the Metropolis scan of every chain over its n_steps + 1 weights, a lane
//                       per chain.
// imhkb_gather_kernel   one wave per chain: the final and the kept states out of the draws, the
//                       final state's lattice point in the defined order.
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
//
// WL (lgs_imhk_bases): the draw's counters are (chain, step) = (a.base + q T C + m / S1, m % S1),
// SampleZ also returns its window log normaliser, and DW takes their sum over the drawn
// coordinates, added for i = d-1 .. 0, instead of the distance.
template <bool WL>
__device__ __forceinline__ void kleinb_draw_body(const KleinbArgs& a) {
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
        if (tid < nl) a.DW[row0 + tid] = WL ? -INFINITY : INFINITY;
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
        CoordStream rs;
        if (WL) {
            const uint64_t c = a.base + (uint64_t)q * (uint64_t)(TK / a.S1) + (uint64_t)(m / a.S1);
            rs.init(a.seed, (uint32_t)(m % a.S1), (uint32_t)c);
        } else {
            const uint64_t s = a.base + (uint64_t)q * (uint64_t)TK + (uint64_t)m;
            rs.init(a.seed, (uint32_t)(s >> 32), (uint32_t)s);
        }
        double D = 0.0;  // WL: the log weight
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
                const SampleZOut o = sample_z(mu, si, a.precision, false, rs.u((uint32_t)(d - 1 - i)), WL, a.etab);
                zi = (double)o.z;
                if (WL) D = D + o.log_norm;
            }
            zs[i * L + tid] = zi;
            if (!WL) {
                const double qz = Ri[i] * zi;
                const double r = t - qz;
                D = D + r * r;
            }
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

__global__ __launch_bounds__(256) void kleinb_draw_kernel(const KleinbArgs a) { kleinb_draw_body<false>(a); }
__global__ __launch_bounds__(256) void kleinb_draw_wl_kernel(const KleinbArgs a) { kleinb_draw_body<true>(a); }

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

// ---- lgs_imhk_bases: the scan.  Chain g of the chunk has the weights LW[g S1 ..]; its state
// starts at draw 0 and step t = 1 .. S1 - 1 takes draw t iff u_t < accept_ratio(lw_t, lw_x),
// u_t = accept_uniform(seed, t, base + g).  A chain of a refused basis: logw -inf, no accepts,
// final_step -1 (its draws are zero rows, so its kept states are draw 0).
constexpr int kScanLanes = 256;

// One lane per chain, the steps in turn (a wave per chain that tests 64 steps at a time and
// resumes behind the first taker of a ballot was 1.3 to 10 times slower: DESIGN.md 6m).
__global__ __launch_bounds__(kScanLanes) void imhkb_scan_kernel(const ImhkbArgs a) {
    const int64_t nc = a.m * a.T * a.C;
    const int64_t g = (int64_t)blockIdx.x * kScanLanes + threadIdx.x;
    if (g >= nc) return;
    const int64_t S = a.S1 - 1;
    const bool bad = a.qr_status[g / (a.T * a.C)] != 0;
    const double* __restrict__ lw = a.LW + g * a.S1;
    const uint32_t chain = (uint32_t)(a.base + (uint64_t)g);
    int64_t cur = 0, acc = 0, keep = 0;
    double lw_x = lw[0];
    for (int64_t t = 1; t <= S; ++t) {
        bool take = false;
        if (!bad) {
            const double lw_y = lw[t];
            take = accept_uniform(a.seed, (uint32_t)t, chain) < accept_ratio(lw_y, lw_x);
            if (take) {
                cur = t;
                lw_x = lw_y;
                ++acc;
            }
        }
        a.accepted[g * S + (t - 1)] = take ? 1 : 0;
        if (a.sel && t % a.thin == 0) a.sel[g * a.n_keep + keep++] = (int32_t)cur;
    }
    a.logw[g] = lw_x;
    a.accepts[g] = acc;
    a.final_step[g] = bad ? -1 : cur;
}

// Wave w of a block is chain g = 4 blockIdx + w; lane i < d carries coordinate i.
__global__ __launch_bounds__(64 * kSelectWaves) void imhkb_gather_kernel(const ImhkbArgs a) {
    const int d = a.d, lane = threadIdx.x & 63;
    const int64_t TC = a.T * a.C;
    const int64_t g = (int64_t)blockIdx.x * kSelectWaves + (threadIdx.x >> 6);
    if (g >= a.m * TC) return;
    const int64_t q = g / TC;
    const bool bad = a.qr_status[q] != 0;
    if (lane == 0 && g % a.C == 0) a.status[g / a.C] = bad ? 3 : 0;
    if (lane >= d) return;
    const size_t src = (size_t)(g * a.S1 + (bad ? 0 : a.final_step[g])) * d;
    const size_t row = (size_t)g * d;
    if (a.zb == 8)
        ((int64_t*)a.z)[row + lane] = ((const int64_t*)a.ZW)[src + lane];
    else
        ((int32_t*)a.z)[row + lane] = ((const int32_t*)a.ZW)[src + lane];
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
    if (!a.zs) return;
    for (int64_t r = 0; r < a.n_keep; ++r) {
        const size_t from = (size_t)(g * a.S1 + a.sel[g * a.n_keep + r]) * d + lane;
        const size_t to = (size_t)(g * a.n_keep + r) * d + lane;
        if (a.zb == 8)
            ((int64_t*)a.zs)[to] = ((const int64_t*)a.ZW)[from];
        else
            ((int32_t*)a.zs)[to] = ((const int32_t*)a.ZW)[from];
    }
}

bool imhkb_args_ok(const ImhkbArgs& a) {
    return a.d >= 2 && a.d <= kCvpMaxD && a.T >= 1 && a.T <= kKleinbMaxT && a.C >= 1 && a.S1 >= 1 && a.m >= 1 &&
           a.m <= kKleinbSlots && (a.zb == 4 || a.zb == 8) && a.thin >= 1 && a.n_keep == (a.S1 - 1) / a.thin &&
           a.m * a.T * a.C * a.S1 <= kKleinbMaxDraws && a.qr_status && a.LW && a.ZW && a.accepted && a.accepts &&
           a.final_step && a.logw;
}

bool kleinb_args_ok(const KleinbArgs& a) {
    return a.d >= 2 && a.d <= kCvpMaxD && a.T >= 1 && a.T <= kKleinbMaxT && a.K >= 1 && a.m >= 1 &&
           a.m <= kKleinbSlots && (a.zb == 4 || a.zb == 8) && (int64_t)a.T * a.K <= kKleinbMaxDraws && a.qr_status &&
           a.ZW && a.DW && a.flags;
}

}  // namespace

namespace launch {

namespace {
hipError_t kleinb_draw_launch(void (*kernel)(const KleinbArgs), const KleinbArgs& a, hipStream_t st) {
    if (!kleinb_args_ok(a) || a.precision < 1 || !a.sigma || !a.R || !a.cprime) return hipErrorInvalidValue;
    const int L = kleinb_lanes(a.d);
    const int64_t TK = (int64_t)a.T * a.K;
    const int64_t grid = a.m * ((TK + L - 1) / L);
    if (grid > 0x7fffffffll) return hipErrorInvalidValue;
    const size_t lds = kleinb_lds_bytes(a.d, a.T, a.K);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(L), lds, st, a);
    return hipGetLastError();
}
}  // namespace

hipError_t kleinb_draw(const KleinbArgs& a, hipStream_t st) { return kleinb_draw_launch(kleinb_draw_kernel, a, st); }

hipError_t kleinb_draw_wl(const KleinbArgs& a, hipStream_t st) {
    if (a.S1 < 1 || a.K % a.S1 != 0) return hipErrorInvalidValue;
    return kleinb_draw_launch(kleinb_draw_wl_kernel, a, st);
}

hipError_t imhkb_scan(const ImhkbArgs& a, hipStream_t st) {
    if (!imhkb_args_ok(a)) return hipErrorInvalidValue;
    const int64_t grid = (a.m * a.T * a.C + kScanLanes - 1) / kScanLanes;
    hipLaunchKernelGGL(imhkb_scan_kernel, dim3((unsigned)grid), dim3(kScanLanes), 0, st, a);
    return hipGetLastError();
}

hipError_t imhkb_gather(const ImhkbArgs& a, hipStream_t st) {
    if (!imhkb_args_ok(a) || !a.bases || !a.z || !a.v || !a.status || (a.zs && !a.sel)) return hipErrorInvalidValue;
    const int64_t grid = (a.m * a.T * a.C + kSelectWaves - 1) / kSelectWaves;
    hipLaunchKernelGGL(imhkb_gather_kernel, dim3((unsigned)grid), dim3(64 * kSelectWaves), 0, st, a);
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
