// lgs_cvpb.hip -- exact closest vectors over a batch of bases (lgs_closest_vector_bases,
// include/lgs.h): every basis brings its own targets, nothing is loaded into
// the context.
//
// cvpb_qr_kernel   one wave per basis: the Householder QR(p) of lgs.h on W = [B_p | targets]
//                  in LDS, a lane owning a column, so every sum of the definition is a
//                  lane-private sequential loop and the result is the definition's bit for bit.
//                  lgs_klein_bases (lgs_kleinb.hip) runs it too, without the search's state.
// cvpb_enum_kernel one wave per basis, lane k its target k: the search of lgs_cvp.hip (the
//                  lane state machine of lgs_cvp_loop.h) on the block's own R.  A launch
//                  advances a problem by at most `slice` nodes, from and to its slot of the
//                  state block, and lists the bases that still have an unfinished problem; the
//                  next launch has one block per listed basis (lgs_lll.hip's live list).  Lanes
//                  are not compacted across bases: a block's LDS holds one R.
// cvpb_finish_kernel  the problems' outputs in the caller's layout, v in the defined order.
//
// All fp64 arithmetic is unfused (the Makefile compiles with -ffp-contract=off); sqrt and
// the division are IEEE-correct.  Control flow of the QR is wave-uniform.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "lgs_cvp_loop.h"
#include "lgs_kernels.h"

namespace lgs {
namespace {

__global__ __launch_bounds__(256) void cvpb_check_kernel(const double* __restrict__ x, int64_t n,
                                                         unsigned int* flags) {
    bool bad = false;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        bad = bad || !isfinite(x[k]);
    if (bad) atomicOr(flags, kFlagNonFinite);
}

// LDS: W, d rows of pitch cvpb_ld(d, T) (odd: a column walk by one lane and a row sweep by the
// wave both spread over the banks).  Columns 0 .. d-1 are B_p, column d + k is target k.  Lane l
// owns columns l and l + 64.  Column k of step k holds the Householder vector v while the other
// columns are updated (v[k] overwrites W[k][k]; the rest of v is the column itself).
__global__ __launch_bounds__(kCvpLanes) void cvpb_qr_kernel(const CvpbArgs a) {
    extern __shared__ double W[];
    const int d = a.d, T = a.T, nc = d + T, ld = cvpb_ld(d, T), lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const double* B = a.bases + (size_t)q * d * d;
    const double* Tg = a.targets + (size_t)q * T * d;
    for (int e = lane; e < d * d; e += kCvpLanes) W[(e / d) * ld + e % d] = B[e];
    for (int e = lane; e < T * d; e += kCvpLanes) W[(e % d) * ld + d + e / d] = Tg[e];
    __syncthreads();
    bool bad = false;
    for (int k = 0; k < d; ++k) {
        double s = 0.0;
        if (lane == 0)
            for (int i = k; i < d; ++i) {
                const double x = W[i * ld + k];
                s = s + x * x;
            }
        s = __shfl(s, 0);
        const double nrm = sqrt(s);
        if (!(nrm > 0.0 && nrm < INFINITY)) {  // (wave-uniform: s is lane 0's)
            bad = true;
            break;
        }
        const double wkk = W[k * ld + k];
        const double alpha = wkk >= 0.0 ? -nrm : nrm;
        __syncthreads();
        double vv = 0.0;
        if (lane == 0) {
            W[k * ld + k] = wkk - alpha;
            for (int i = k; i < d; ++i) {
                const double x = W[i * ld + k];
                vv = vv + x * x;
            }
        }
        vv = __shfl(vv, 0);
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int c = lane + pass * kCvpLanes;
            if (c > k && c < nc) {
                double dot = 0.0;
                for (int i = k; i < d; ++i) dot = dot + W[i * ld + k] * W[i * ld + c];
                const double f = (dot + dot) / vv;
                for (int i = k; i < d; ++i) W[i * ld + c] = W[i * ld + c] - f * W[i * ld + k];
            }
        }
        __syncthreads();
        if (lane == 0) W[k * ld + k] = alpha;
        for (int i = k + 1 + lane; i < d; i += kCvpLanes) W[i * ld + k] = 0.0;
        __syncthreads();
    }
    if (!bad) {  // rows with a negative diagonal are negated, from the diagonal on
        const unsigned long long neg = __ballot(lane < d && W[lane * ld + lane] < 0.0);
        __syncthreads();
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int c = lane + pass * kCvpLanes;
            if (c < nc)
                for (int k = 0; k < d && k <= c; ++k)
                    if ((neg >> k) & 1ull) W[k * ld + c] = -W[k * ld + c];
        }
        __syncthreads();
    }
    double* Ro = a.R + (size_t)q * d * d;
    for (int e = lane; e < d * d; e += kCvpLanes) Ro[e] = bad ? 0.0 : W[(e / d) * ld + e % d];
    double* co = a.cprime + (size_t)q * T * d;
    for (int e = lane; e < T * d; e += kCvpLanes) co[e] = bad ? 0.0 : W[(e % d) * ld + d + e / d];
    if (lane == 0) a.qr_status[q] = bad ? 3 : 0;
    if (!a.CP) return;  // (cvpb_qr_only: no search follows, no centre store and no state block)
    double* CPo = a.CP + (size_t)q * d * kCvpLanes;
    for (int i = 0; i < d; ++i) CPo[i * kCvpLanes + lane] = (bad || lane >= T) ? 0.0 : W[i * ld + d + lane];
    const int64_t s = q * kCvpLanes + lane;
    a.st.tgt[s] = (bad || lane >= T) ? kCvpbDone : kCvpbFresh;
    a.st.lvl[s] = 0;
    a.st.has_best[s] = 0;
    a.st.A[s] = INFINITY;
    a.st.nodes[s] = 0;
    a.pstatus[s] = bad ? 3 : 0;
}

// LDS of a block: R_q (d x d), then base | P | z | sn of its lanes, cvp_enum_kernel's layout.
__global__ __launch_bounds__(kCvpLanes) void cvpb_enum_kernel(const CvpbArgs a) {
    extern __shared__ double lds[];
    const int d = a.d, lane = threadIdx.x;
    const int64_t q = a.live_in ? (int64_t)a.live_in[blockIdx.x] : (int64_t)blockIdx.x;
    double* Rs = lds;
    const double* Rq = a.R + (size_t)q * d * d;
    for (int k = lane; k < d * d; k += kCvpLanes) Rs[k] = Rq[k];
    __syncthreads();
    const int64_t S = a.S;
    const int64_t s = q * kCvpLanes + lane;
    double* base = lds + d * d + lane;
    double* P = base + d * kCvpLanes;
    double* z = P + d * kCvpLanes;
    double* sn = z + d * kCvpLanes;
    int64_t* best = a.st.best + s;
    const double* cpt = a.CP + (size_t)q * d * kCvpLanes + lane;
    const int64_t ldc = kCvpLanes;
    const int phase0 = a.st.tgt[s];
    int phase = phase0, status = 0;
    int i = a.st.lvl[s];
    int hb = a.st.has_best[s];
    double A = a.st.A[s];
    int64_t nodes = a.st.nodes[s];
    if (phase == kCvpbFresh) {
        bool ok = true;
        for (int k = 0; k < d; ++k) ok = ok && isfinite(cpt[(size_t)k * ldc]);
        A = a.radius2 ? a.radius2[q * a.T + lane] : INFINITY;
        i = d - 1;
        if (ok) ok = cvp_enter(Rs, d, i, cpt, ldc, z, base, sn);
        phase = kCvpbRunning;
        if (!ok) {
            atomicOr(a.flags, kFlagNonFinite);
            status = 2;
            phase = kCvpbDone;
        }
    } else if (phase == kCvpbRunning) {
        for (int k = 0; k < d; ++k) {
            base[k * kCvpLanes] = a.st.base[(size_t)k * S + s];
            P[k * kCvpLanes] = a.st.P[(size_t)k * S + s];
            z[k * kCvpLanes] = a.st.z[(size_t)k * S + s];
            sn[k * kCvpLanes] = a.st.sn[(size_t)k * S + s];
        }
    }
    int64_t budget = a.slice;
    while (phase == kCvpbRunning) {
        if (nodes == a.max_nodes) {  // the best found so far, unproven
            status = 1;
            phase = kCvpbDone;
            break;
        }
        if (budget == 0) break;
        ++nodes;
        --budget;
        const CvpStep e = cvp_step(Rs, d, cpt, ldc, z, base, P, sn, best, S, i, hb, A);
        if (e == kCvpBad) {
            atomicOr(a.flags, kFlagNonFinite);
            status = 2;
            hb = 0;
            phase = kCvpbDone;
        } else if (e == kCvpDone) {
            status = hb ? 0 : 2;
            phase = kCvpbDone;
        }
    }
    if (phase0 != kCvpbDone) {
        a.st.tgt[s] = phase;
        a.st.lvl[s] = i;
        a.st.has_best[s] = hb;
        a.st.A[s] = A;
        a.st.nodes[s] = nodes;
        if (phase == kCvpbDone) {
            a.pstatus[s] = status;
        } else {
            for (int k = 0; k < d; ++k) {
                a.st.base[(size_t)k * S + s] = base[k * kCvpLanes];
                a.st.P[(size_t)k * S + s] = P[k * kCvpLanes];
                a.st.z[(size_t)k * S + s] = z[k * kCvpLanes];
                a.st.sn[(size_t)k * S + s] = sn[k * kCvpLanes];
            }
        }
    }
    const unsigned long long live = __ballot(phase == kCvpbRunning);
    if (lane == 0 && live) {
        const unsigned long long at = atomicAdd(a.ctl, 1ull);
        if (at < (unsigned long long)a.nlive) a.live_out[at] = (int32_t)q;
    }
}

// One block per basis, lane k its problem k.  LDS: the lanes' coefficients, (j, lane) at
// [j * kCvpLanes + lane].  v[i] = sum over ascending j of bases[p][i][j] * (double)z[j].
template <typename OT>
__global__ __launch_bounds__(kCvpLanes) void cvpb_finish_kernel(const CvpbArgs a) {
    extern __shared__ double zs[];
    const int d = a.d, T = a.T, lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    if (lane >= T) return;
    const int64_t S = a.S;
    const int64_t s = q * kCvpLanes + lane;
    const int hb = a.st.has_best[s];
    const size_t row = ((size_t)q * T + lane) * d;
    OT* zo = (OT*)a.z + row;
    bool over = false;
    for (int j = 0; j < d; ++j) {
        const int64_t v = hb ? a.st.best[(size_t)j * S + s] : 0;
        if (sizeof(OT) == 4 && (v >= (1ll << 31) || v <= -(1ll << 31))) over = true;
        zo[j] = (OT)v;
        zs[j * kCvpLanes + lane] = (double)v;
    }
    if (over) atomicOr(a.flags, kFlagOverflow);
    const double* B = a.bases + (size_t)q * d * d;
    double* vo = a.v + row;
    for (int i = 0; i < d; ++i) {
        double acc = 0.0;
        for (int j = 0; j < d; ++j) acc = acc + B[i * d + j] * zs[j * kCvpLanes + lane];
        vo[i] = acc;
    }
    a.dist2[q * T + lane] = hb ? a.st.A[s] : INFINITY;
    a.nodes[q * T + lane] = a.st.nodes[s];
    a.status[q * T + lane] = a.pstatus[s];
}

hipError_t cvpb_args_ok(const CvpbArgs& a) {
    if (a.d < 2 || a.d > kCvpMaxD || a.T < 1 || a.T > kCvpbMaxT || a.m < 1 || a.m * kCvpLanes > a.S || !a.R || !a.CP ||
        !a.st.z || !a.pstatus || !a.flags)
        return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t big_lds(const void* fn, size_t lds) {
    if (lds <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

}  // namespace

namespace launch {

hipError_t cvpb_check(const double* x, int64_t n, unsigned int* flags, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!x || !flags) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(cvpb_check_kernel, dim3(grid), dim3(256), 0, st, x, n, flags);
    return hipGetLastError();
}

hipError_t cvpb_qr(const CvpbArgs& a, hipStream_t st) {
    hipError_t e = cvpb_args_ok(a);
    if (e != hipSuccess) return e;
    if (!a.bases || !a.targets || !a.cprime || !a.qr_status) return hipErrorInvalidValue;
    const size_t lds = cvpb_qr_lds_bytes(a.d, a.T);
    if ((e = big_lds((const void*)cvpb_qr_kernel, lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(cvpb_qr_kernel, dim3((unsigned)a.m), dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t cvpb_qr_only(const CvpbArgs& a, hipStream_t st) {
    if (a.d < 2 || a.d > kCvpMaxD || a.T < 1 || a.T > kCvpbMaxT || a.m < 1 || a.CP) return hipErrorInvalidValue;
    if (!a.bases || !a.targets || !a.R || !a.cprime || !a.qr_status) return hipErrorInvalidValue;
    const size_t lds = cvpb_qr_lds_bytes(a.d, a.T);
    const hipError_t e = big_lds((const void*)cvpb_qr_kernel, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cvpb_qr_kernel, dim3((unsigned)a.m), dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t cvpb_enum(const CvpbArgs& a, hipStream_t st) {
    if (a.nlive <= 0) return hipSuccess;
    hipError_t e = cvpb_args_ok(a);
    if (e != hipSuccess) return e;
    if (a.nlive > a.m || !a.live_out || !a.ctl || a.slice < 1 || a.max_nodes < 1) return hipErrorInvalidValue;
    const size_t lds = cvp_lds_bytes(a.d);  // up to the CU's whole 160 KiB at d = 64
    if ((e = big_lds((const void*)cvpb_enum_kernel, lds)) != hipSuccess) return e;
    hipLaunchKernelGGL(cvpb_enum_kernel, dim3((unsigned)a.nlive), dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t cvpb_finish(const CvpbArgs& a, int zb, hipStream_t st) {
    hipError_t e = cvpb_args_ok(a);
    if (e != hipSuccess) return e;
    if (!a.bases || !a.z || !a.v || !a.dist2 || !a.nodes || !a.status || (zb != 4 && zb != 8))
        return hipErrorInvalidValue;
    const size_t lds = (size_t)a.d * kCvpLanes * 8;
    if (zb == 8)
        hipLaunchKernelGGL(cvpb_finish_kernel<int64_t>, dim3((unsigned)a.m), dim3(kCvpLanes), lds, st, a);
    else
        hipLaunchKernelGGL(cvpb_finish_kernel<int32_t>, dim3((unsigned)a.m), dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
