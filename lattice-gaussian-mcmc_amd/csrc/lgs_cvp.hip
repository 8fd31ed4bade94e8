// lgs_cvp.hip -- exact closest-vector decoding: Schnorr-Euchner enumeration in the QR
// frame (lgs_closest_vector, include/lgs.h).
//
// One target per lane, run as a level state machine: the lane stands on level i of its
// target's tree, visits one node per iteration (descend, improve the bound at level 0, or
// prune and step to the parent's next sibling) and keeps everything it needs to resume in
// the device state block (CvpState), so no launch is unbounded: a launch ends after `slice`
// nodes per lane, and the host relaunches until every target has stopped.  A lane whose
// target stops takes the next waiting target of the chunk inside the same launch.
//
// The arithmetic is the operational definition of lgs.h, fp64 and unfused (the Makefile
// compiles with -ffp-contract=off), every sum in the reference's order, so the traversal --
// and with it z, dist2, nodes and status -- is the same whatever the slice, the slot a
// target lands in or the chunk it belongs to.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"

namespace lgs {
namespace {

// enter(i): the level's conditional centre from the coefficients above it, the nearest
// integer and the side the zig-zag starts on.  false: the mean is not finite (or beyond
// 2^52), the search of this target cannot go on.  z / base / sn: the lane's columns of the
// block's LDS arrays (element i at [i * kCvpLanes]).
__device__ inline bool cvp_enter(const double* Rs, int d, int i, const double* cpt, int64_t ldc, double* z,
                                 double* base, double* sn) {
    const double* Ri = Rs + i * d;
    double cs = 0.0;
    int j = i + 1;
    // (eight LDS reads of each operand in flight per round trip; the sum keeps its order)
    for (; j + 8 <= d; j += 8) {
        double rr[8];
        double zz[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            rr[u] = Ri[j + u];
            zz[u] = z[(j + u) * kCvpLanes];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) cs = cs + rr[u] * zz[u];
    }
    if (j + 4 <= d) {
        double rr[4];
        double zz[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rr[u] = Ri[j + u];
            zz[u] = z[(j + u) * kCvpLanes];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) cs = cs + rr[u] * zz[u];
        j += 4;
    }
    for (; j < d; ++j) cs = cs + Ri[j] * z[j * kCvpLanes];
    const double b = cpt[(size_t)i * ldc] - cs;
    const double m = b / Ri[i];
    const double zr = rint(m);
    if (!(fabs(m) < kCvpMaxAbsZ)) return false;
    base[i * kCvpLanes] = b;
    z[i * kCvpLanes] = zr;
    sn[i * kCvpLanes] = m >= zr ? 1.0 : -1.0;
    return true;
}

template <typename OT>
__device__ inline void cvp_finish(const CvpArgs& a, int64_t t, int status, int hb, double A, int64_t nodes,
                                  const int64_t* best) {
    OT* W = (OT*)a.W;
    bool over = false;
    for (int k = 0; k < a.d; ++k) {
        const int64_t v = hb ? best[(size_t)k * a.S] : 0;
        if (sizeof(OT) == 4 && (v >= (1ll << 31) || v <= -(1ll << 31))) over = true;
        W[(size_t)k * a.ldw + t] = (OT)v;
    }
    if (over) atomicOr(a.flags, kFlagOverflow);
    a.dist2[t] = hb ? A : INFINITY;
    a.nodes[t] = nodes;
    a.status[t] = status;
}

// Coefficients and zig-zag offsets are held as doubles: integers below 2^53 in magnitude
// (a mean of 2^52 or more ends the target's search, and a search moves a coefficient by at
// most max_nodes <= 2^40), so every value and every z += offset is exact and the products
// R_ij z_j need no integer conversion in the loop.
// LDS of a block (one wave, kCvpLanes lanes): R (d x d), then the lanes' working state
// base | P | z | sn, each d x kCvpLanes 8-byte elements with element (i, lane) at
// [i * kCvpLanes + lane] -- conflict-free whatever level each lane stands on.  A lane's
// columns are loaded from its slot of the state block when the launch starts and stored
// back when it ends; the best point stays in the state block (written on improvements only).
template <typename OT>
__global__ __launch_bounds__(kCvpLanes) void cvp_enum_kernel(const CvpArgs a) {
    extern __shared__ double lds[];
    const int d = a.d;
    double* Rs = lds;
    for (int k = threadIdx.x; k < d * d; k += kCvpLanes) Rs[k] = a.R[k];
    __syncthreads();
    const int64_t s = (int64_t)blockIdx.x * kCvpLanes + threadIdx.x;
    if (s >= a.nslots) return;
    const int64_t S = a.S;
    double* base = lds + d * d + threadIdx.x;
    double* P = base + d * kCvpLanes;
    double* z = P + d * kCvpLanes;
    double* sn = z + d * kCvpLanes;
    int64_t* best = a.st.best + s;
    int64_t t = a.st.tgt[s];
    int i = a.st.lvl[s];
    int hb = a.st.has_best[s];
    double A = a.st.A[s];
    int64_t nodes = a.st.nodes[s];
    if (t >= 0)
        for (int k = 0; k < d; ++k) {
            base[k * kCvpLanes] = a.st.base[(size_t)k * S + s];
            P[k * kCvpLanes] = a.st.P[(size_t)k * S + s];
            z[k * kCvpLanes] = a.st.z[(size_t)k * S + s];
            sn[k * kCvpLanes] = a.st.sn[(size_t)k * S + s];
        }
    int64_t budget = a.slice;
    for (;;) {
        if (t < 0) {  // idle: the next waiting target of the chunk
            if (*(volatile unsigned long long*)a.ctl >= (unsigned long long)a.m) break;
            const unsigned long long q = atomicAdd(a.ctl, 1ull);
            if (q >= (unsigned long long)a.m) break;
            t = (int64_t)q;
            bool ok = true;
            for (int k = 0; k < d; ++k) ok = ok && isfinite(a.CP[(size_t)k * a.ldc + t]);
            A = a.radius2 ? a.radius2[t] : INFINITY;
            hb = 0;
            nodes = 0;
            i = d - 1;
            if (ok) ok = cvp_enter(Rs, d, i, a.CP + t, a.ldc, z, base, sn);
            if (!ok) {
                atomicOr(a.flags, kFlagNonFinite);
                cvp_finish<OT>(a, t, 2, 0, A, nodes, best);
                t = -1;
                continue;
            }
        }
        if (budget == 0) break;
        if (nodes == a.max_nodes) {  // the best found so far, unproven
            cvp_finish<OT>(a, t, 1, hb, A, nodes, best);
            t = -1;
            continue;
        }
        ++nodes;
        --budget;
        const double r = base[i * kCvpLanes] - Rs[i * d + i] * z[i * kCvpLanes];
        const double Pi = (i == d - 1 ? 0.0 : P[(i + 1) * kCvpLanes]) + r * r;
        if (Pi < A) {
            if (i == 0) {  // a closer point; its siblings at level 0 follow
                A = Pi;
                hb = 1;
                for (int k = 0; k < d; ++k) best[(size_t)k * S] = (int64_t)z[k * kCvpLanes];
            } else {
                P[i * kCvpLanes] = Pi;
                --i;
                if (!cvp_enter(Rs, d, i, a.CP + t, a.ldc, z, base, sn)) {
                    atomicOr(a.flags, kFlagNonFinite);
                    cvp_finish<OT>(a, t, 2, 0, A, nodes, best);
                    t = -1;
                }
                continue;
            }
        } else {  // every further sibling of this level is farther: back to the parent's next one
            ++i;
            if (i == d) {
                cvp_finish<OT>(a, t, hb ? 0 : 2, hb, A, nodes, best);
                t = -1;
                continue;
            }
        }
        const double w = sn[i * kCvpLanes];  // next sibling: z += stp * (nxt + 1), the side flips
        z[i * kCvpLanes] += w;
        sn[i * kCvpLanes] = -(w + (w > 0.0 ? 1.0 : -1.0));
    }
    a.st.tgt[s] = (int32_t)t;
    a.st.lvl[s] = i;
    a.st.has_best[s] = hb;
    a.st.A[s] = A;
    a.st.nodes[s] = nodes;
    if (t >= 0) {
        for (int k = 0; k < d; ++k) {
            a.st.base[(size_t)k * S + s] = base[k * kCvpLanes];
            a.st.P[(size_t)k * S + s] = P[k * kCvpLanes];
            a.st.z[(size_t)k * S + s] = z[k * kCvpLanes];
            a.st.sn[(size_t)k * S + s] = sn[k * kCvpLanes];
        }
        atomicAdd(a.ctl + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void cvp_compact_kernel(const CvpState src, const CvpState dst, int64_t S,
                                                          const int32_t* __restrict__ map, int64_t nlive) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nlive) return;
    const int64_t s = map[q];
    const size_t k = blockIdx.y;
    dst.z[k * S + q] = src.z[k * S + s];
    dst.base[k * S + q] = src.base[k * S + s];
    dst.P[k * S + q] = src.P[k * S + s];
    dst.sn[k * S + q] = src.sn[k * S + s];
    dst.best[k * S + q] = src.best[k * S + s];
    if (k == 0) {
        dst.A[q] = src.A[s];
        dst.nodes[q] = src.nodes[s];
        dst.tgt[q] = src.tgt[s];
        dst.lvl[q] = src.lvl[s];
        dst.has_best[q] = src.has_best[s];
    }
}

}  // namespace

namespace launch {

hipError_t cvp_enum(const CvpArgs& a, int zb, hipStream_t st) {
    if (a.nslots <= 0) return hipSuccess;
    if (a.d < 1 || a.d > kCvpMaxD || a.nslots > a.S || a.m > a.ldc || a.m > a.ldw) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nslots + kCvpLanes - 1) / kCvpLanes));
    const size_t lds = cvp_lds_bytes(a.d);  // up to the CU's whole 160 KiB at d = 64
    const void* fn = zb == 8 ? (const void*)cvp_enum_kernel<int64_t> : (const void*)cvp_enum_kernel<int32_t>;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (zb == 8)
        hipLaunchKernelGGL(cvp_enum_kernel<int64_t>, grid, dim3(kCvpLanes), lds, st, a);
    else
        hipLaunchKernelGGL(cvp_enum_kernel<int32_t>, grid, dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t cvp_compact(const CvpState& src, const CvpState& dst, int64_t S, const int32_t* map, int64_t nlive,
                       int d, hipStream_t st) {
    if (nlive <= 0) return hipSuccess;
    if (nlive > S) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nlive + 255) / 256), (unsigned)d);
    hipLaunchKernelGGL(cvp_compact_kernel, grid, dim3(256), 0, st, src, dst, S, map, nlive);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
