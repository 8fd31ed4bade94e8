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

#include "lgs_cvp_loop.h"
#include "lgs_kernels.h"

namespace lgs {
namespace {

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
        const CvpStep e = cvp_step(Rs, d, a.CP + t, a.ldc, z, base, P, sn, best, S, i, hb, A);
        if (e == kCvpBad) {
            atomicOr(a.flags, kFlagNonFinite);
            cvp_finish<OT>(a, t, 2, 0, A, nodes, best);
            t = -1;
        } else if (e == kCvpDone) {
            cvp_finish<OT>(a, t, hb ? 0 : 2, hb, A, nodes, best);
            t = -1;
        }
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

// ---- exact Gaussian mass: the same search with a fixed bound and a weight on every leaf
// (lgs_gaussian_mass, include/lgs.h).
//
// A work item is a partial tree (target, top, prefix): the lane starts on level top - 1
// under the node z[top .. d-1] whose partial distance is P[top], visits the nodes the
// unsplit traversal visits below that node, with the same arithmetic, and stops when it
// climbs back to `top`.  The bound A = radius2 never changes, so items do not depend on
// each other.  Every point with D < A is counted with w = exp((shift - D) / 2 sigma^2).
//
// sum_z (MOMENTS) costs O(1) per node: msub[i] is the weight of the points below the
// current node of level i.  A leaf adds w to msub[1] and z_0 w to S[0]; when the lane climbs
// from level i - 1 to level i, S[i] += z_i msub[i], msub[i+1] += msub[i], msub[i] = 0.  The
// item's own mass stands for msub[top], which the host folds into the levels of the prefix.

__device__ inline void mass_finish(const MassArgs& a, int64_t q, int status, double mass, double energy,
                                   double dmin, int64_t points, int64_t nodes, const double* Sz, bool moments) {
    a.o_mass[q] = mass;
    a.o_energy[q] = energy;
    a.o_dmin[q] = dmin;
    a.o_points[q] = points;
    a.o_nodes[q] = nodes;
    a.o_status[q] = status;
    if (moments)
        for (int k = 0; k < a.d; ++k) a.o_sz[(size_t)k * a.ldo + q] = k < a.top ? Sz[k * kCvpLanes] : 0.0;
}

// The listing pass: the point's row, full coefficients and D.  The row number comes from the
// counting pass over the same items, so it is below l_rows; the test keeps a store inside the
// buffers whatever the counts say.
__device__ inline void mass_list_row(const MassArgs& a, int64_t row, const double* z, double D) {
    if ((unsigned long long)row >= (unsigned long long)a.l_rows) return;
    a.l_d[row] = D;
    if (a.l_zb == 8) {
        int64_t* o = (int64_t*)a.l_z + (size_t)row * a.d;
        for (int k = 0; k < a.d; ++k) o[k] = (int64_t)z[k * kCvpLanes];
    } else {
        int32_t* o = (int32_t*)a.l_z + (size_t)row * a.d;
        bool over = false;
        for (int k = 0; k < a.d; ++k) {
            const int64_t v = (int64_t)z[k * kCvpLanes];
            if (v >= (1ll << 31) || v <= -(1ll << 31)) over = true;
            o[k] = (int32_t)v;
        }
        if (over) atomicOr(a.flags, kFlagOverflow);
    }
}

// LDS of a block: R (d x d), then base | P | z | sn (| msub | S) of its lanes, laid out as
// cvp_enum_kernel's.  The sums and counts of the item live in registers between the nodes
// and in the state block between the launches.  LIST (never with MOMENTS): the listing pass
// of lgs_ball_points -- the same nodes, every point written as row it_first[item] + (points
// of the item so far) instead of summed; the running count is the state's `points`, so
// slicing, the hand-out of waiting items and compaction are the counting pass's.
template <bool MOMENTS, bool LIST>
__global__ __launch_bounds__(kCvpLanes) void mass_enum_kernel(const MassArgs a) {
    extern __shared__ double lds[];
    const int d = a.d;
    const int top = a.top;
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
    double* msub = sn + d * kCvpLanes;   // (MOMENTS only: the LDS ends at sn otherwise)
    double* Sz = msub + d * kCvpLanes;
    int64_t q = a.st.item[s];
    int i = a.st.lvl[s];
    double mass = a.st.mass[s];
    double energy = a.st.energy[s];
    double dmin = a.st.dmin[s];
    int64_t points = a.st.points[s];
    int64_t nodes = a.st.nodes[s];
    int64_t t = -1;
    double A = 0.0, sh = 0.0;
    if (q >= 0) {
        t = a.it_tgt ? a.it_tgt[q] : q;
        A = a.radius2[t];
        sh = a.shift ? a.shift[t] : 0.0;
        for (int k = 0; k < d; ++k) {
            base[k * kCvpLanes] = a.st.base[(size_t)k * S + s];
            P[k * kCvpLanes] = a.st.P[(size_t)k * S + s];
            z[k * kCvpLanes] = a.st.z[(size_t)k * S + s];
            sn[k * kCvpLanes] = a.st.sn[(size_t)k * S + s];
            if (MOMENTS) {
                msub[k * kCvpLanes] = a.st.msub[(size_t)k * S + s];
                Sz[k * kCvpLanes] = a.st.Sz[(size_t)k * S + s];
            }
        }
    }
    int64_t budget = a.slice;
    for (;;) {
        if (q < 0) {  // idle: the next waiting item of the chunk
            if (*(volatile unsigned long long*)a.ctl >= (unsigned long long)a.m) break;
            const unsigned long long nq = atomicAdd(a.ctl, 1ull);
            if (nq >= (unsigned long long)a.m) break;
            q = (int64_t)nq;
            t = a.it_tgt ? a.it_tgt[q] : q;
            A = a.radius2[t];
            sh = a.shift ? a.shift[t] : 0.0;
            bool ok = true;
            for (int k = 0; k < d; ++k) ok = ok && isfinite(a.CP[(size_t)k * a.ldc + t]);
            mass = 0.0;
            energy = 0.0;
            dmin = INFINITY;
            points = 0;
            nodes = 0;
            for (int k = 0; k < d; ++k) {
                base[k * kCvpLanes] = 0.0;
                sn[k * kCvpLanes] = 0.0;
                P[k * kCvpLanes] = k == top ? a.it_P[q] : 0.0;
                z[k * kCvpLanes] = k >= top ? a.it_z[(size_t)(k - top) * a.ldi + q] : 0.0;
                if (MOMENTS) {
                    msub[k * kCvpLanes] = 0.0;
                    Sz[k * kCvpLanes] = 0.0;
                }
            }
            i = top - 1;
            if (ok) ok = cvp_enter(Rs, d, i, a.CP + t, a.ldc, z, base, sn);
            if (!ok) {
                atomicOr(a.flags, kFlagNonFinite);
                mass_finish(a, q, 2, mass, energy, dmin, points, nodes, Sz, MOMENTS);
                q = -1;
                continue;
            }
        }
        if (budget == 0) break;
        if (nodes == a.max_nodes) {  // the points counted so far: lower bounds
            if (MOMENTS) {  // the open subtrees along the path z[1 .. top-1], so that sum_z covers those points
                double run = 0.0;
                for (int k = 1; k < top; ++k) {
                    run = run + msub[k * kCvpLanes];
                    Sz[k * kCvpLanes] = Sz[k * kCvpLanes] + z[k * kCvpLanes] * run;
                }
            }
            mass_finish(a, q, 1, mass, energy, dmin, points, nodes, Sz, MOMENTS);
            q = -1;
            continue;
        }
        ++nodes;
        --budget;
        const double r = base[i * kCvpLanes] - Rs[i * d + i] * z[i * kCvpLanes];
        const double Pi = (i == d - 1 ? 0.0 : P[(i + 1) * kCvpLanes]) + r * r;
        if (Pi < A) {
            if (i == 0) {  // a point of the ball; its siblings at level 0 follow
                if constexpr (LIST) {
                    mass_list_row(a, a.it_first[q] + points, z, Pi);
                    ++points;
                    dmin = fmin(dmin, Pi);
                } else {
                    const double w = exp((sh - Pi) / a.two_s2);
                    ++points;
                    dmin = fmin(dmin, Pi);
                    mass = mass + w;
                    energy = energy + w * Pi;
                    if (MOMENTS) {
                        if (top > 1) msub[kCvpLanes] = msub[kCvpLanes] + w;
                        Sz[0] = Sz[0] + z[0] * w;
                    }
                }
            } else {
                P[i * kCvpLanes] = Pi;
                --i;
                if (!cvp_enter(Rs, d, i, a.CP + t, a.ldc, z, base, sn)) {
                    atomicOr(a.flags, kFlagNonFinite);
                    mass_finish(a, q, 2, mass, energy, dmin, points, nodes, Sz, MOMENTS);
                    q = -1;
                }
                continue;
            }
        } else {  // every further sibling of this level is outside the ball
            ++i;
            if (i == top) {
                mass_finish(a, q, 0, mass, energy, dmin, points, nodes, Sz, MOMENTS);
                q = -1;
                continue;
            }
            if (MOMENTS) {  // the subtree of the node being left at level i is complete
                const double ms = msub[i * kCvpLanes];
                Sz[i * kCvpLanes] = Sz[i * kCvpLanes] + z[i * kCvpLanes] * ms;
                if (i + 1 < top) msub[(i + 1) * kCvpLanes] = msub[(i + 1) * kCvpLanes] + ms;
                msub[i * kCvpLanes] = 0.0;
            }
        }
        const double w = sn[i * kCvpLanes];
        z[i * kCvpLanes] += w;
        sn[i * kCvpLanes] = -(w + (w > 0.0 ? 1.0 : -1.0));
    }
    a.st.item[s] = (int32_t)q;
    a.st.lvl[s] = i;
    a.st.mass[s] = mass;
    a.st.energy[s] = energy;
    a.st.dmin[s] = dmin;
    a.st.points[s] = points;
    a.st.nodes[s] = nodes;
    if (q >= 0) {
        for (int k = 0; k < d; ++k) {
            a.st.base[(size_t)k * S + s] = base[k * kCvpLanes];
            a.st.P[(size_t)k * S + s] = P[k * kCvpLanes];
            a.st.z[(size_t)k * S + s] = z[k * kCvpLanes];
            a.st.sn[(size_t)k * S + s] = sn[k * kCvpLanes];
            if (MOMENTS) {
                a.st.msub[(size_t)k * S + s] = msub[k * kCvpLanes];
                a.st.Sz[(size_t)k * S + s] = Sz[k * kCvpLanes];
            }
        }
        atomicAdd(a.ctl + 1, 1ull);
    }
}

__global__ __launch_bounds__(256) void mass_compact_kernel(const MassState src, const MassState dst, int64_t S,
                                                           const int32_t* __restrict__ map, int64_t nlive,
                                                           int moments) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nlive) return;
    const int64_t s = map[q];
    const size_t k = blockIdx.y;
    dst.z[k * S + q] = src.z[k * S + s];
    dst.base[k * S + q] = src.base[k * S + s];
    dst.P[k * S + q] = src.P[k * S + s];
    dst.sn[k * S + q] = src.sn[k * S + s];
    if (moments) {
        dst.msub[k * S + q] = src.msub[k * S + s];
        dst.Sz[k * S + q] = src.Sz[k * S + s];
    }
    if (k == 0) {
        dst.mass[q] = src.mass[s];
        dst.energy[q] = src.energy[s];
        dst.dmin[q] = src.dmin[s];
        dst.points[q] = src.points[s];
        dst.nodes[q] = src.nodes[s];
        dst.item[q] = src.item[s];
        dst.lvl[q] = src.lvl[s];
    }
}

}  // namespace

namespace launch {

hipError_t mass_enum(const MassArgs& a, bool moments, hipStream_t st) {
    if (a.nslots <= 0) return hipSuccess;
    if (a.d < 1 || a.d > kMassMaxD || (moments && a.d > kMassMomentsMaxD) || a.top < 1 || a.top > a.d ||
        a.nslots > a.S || a.m > a.ldo || (a.top < a.d && (a.m > a.ldi || !a.it_z || !a.it_P || !a.it_tgt)) ||
        (!a.it_tgt && a.m > a.ldc) || !a.radius2)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nslots + kCvpLanes - 1) / kCvpLanes));
    const size_t lds = mass_lds_bytes(a.d, moments);  // 160 KiB at d = 64; 135 680 B at d = 40 with moments
    const void* fn =
        moments ? (const void*)mass_enum_kernel<true, false> : (const void*)mass_enum_kernel<false, false>;
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (moments)
        hipLaunchKernelGGL((mass_enum_kernel<true, false>), grid, dim3(kCvpLanes), lds, st, a);
    else
        hipLaunchKernelGGL((mass_enum_kernel<false, false>), grid, dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t mass_list(const MassArgs& a, hipStream_t st) {
    if (a.nslots <= 0) return hipSuccess;
    if (a.d < 1 || a.d > kMassMaxD || a.top < 1 || a.top > a.d || a.nslots > a.S || a.m > a.ldo ||
        (a.top < a.d && (a.m > a.ldi || !a.it_z || !a.it_P)) || !a.it_tgt || !a.radius2 || !a.it_first ||
        !a.l_z || !a.l_d || (a.l_zb != 4 && a.l_zb != 8) || a.l_rows < 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nslots + kCvpLanes - 1) / kCvpLanes));
    const size_t lds = mass_lds_bytes(a.d, false);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)mass_enum_kernel<false, true>,
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((mass_enum_kernel<false, true>), grid, dim3(kCvpLanes), lds, st, a);
    return hipGetLastError();
}

hipError_t mass_compact(const MassState& src, const MassState& dst, int64_t S, const int32_t* map, int64_t nlive,
                        int d, bool moments, hipStream_t st) {
    if (nlive <= 0) return hipSuccess;
    if (nlive > S) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((nlive + 255) / 256), (unsigned)d);
    hipLaunchKernelGGL(mass_compact_kernel, grid, dim3(256), 0, st, src, dst, S, map, nlive, moments ? 1 : 0);
    return hipGetLastError();
}

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
