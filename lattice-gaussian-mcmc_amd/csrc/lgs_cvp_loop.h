// lgs_cvp_loop.h -- the lane state machine of the Schnorr-Euchner search (include/lgs.h,
// lgs_closest_vector), shared by cvp_enum_kernel and mass_enum_kernel (lgs_cvp.hip: one
// loaded basis, one target per lane) and cvpb_enum_kernel (lgs_cvpb.hip: one basis per
// block).  Device code only; every includer is compiled with -ffp-contract=off.
//
// A lane's working state lives in its columns of the block's LDS arrays base | P | z | sn,
// element i at [i * kCvpLanes]; Rs is the block's copy of R, row-major d x d.
#pragma once

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

// One node of the search (the body of lgs.h's loop after `nodes += 1`): the lane stands on
// level i with the bound A.  kCvpGo: the search goes on (i, A, hb and the LDS columns are
// updated; an improvement stores the point into best[k * S]).  kCvpDone: the lane climbed
// past level d - 1, the tree is exhausted.  kCvpBad: the mean of the level entered is not
// finite or not below 2^52.
enum CvpStep { kCvpGo = 0, kCvpDone = 1, kCvpBad = 2 };
__device__ inline CvpStep cvp_step(const double* Rs, int d, const double* cpt, int64_t ldc, double* z, double* base,
                                   double* P, double* sn, int64_t* best, int64_t S, int& i, int& hb, double& A) {
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
            return cvp_enter(Rs, d, i, cpt, ldc, z, base, sn) ? kCvpGo : kCvpBad;
        }
    } else {  // every further sibling of this level is farther: back to the parent's next one
        ++i;
        if (i == d) return kCvpDone;
    }
    const double w = sn[i * kCvpLanes];  // next sibling: z += stp * (nxt + 1), the side flips
    z[i * kCvpLanes] += w;
    sn[i * kCvpLanes] = -(w + (w > 0.0 ? 1.0 : -1.0));
    return kCvpGo;
}

}  // namespace
}  // namespace lgs
