// lgs_bkz.hip -- batched BKZ basis reduction (lgs_bkz_reduce, include/lgs.h).
//
// One basis per block of one wave, on the LDS image of lgs_lll.hip (b, U, the exact Gram matrix,
// mu, r[i][i]) extended by the state of the tour and of the block enumeration in work
// (lgs_kernels.h).  The kernel is a state machine of three phases, all control flow wave-uniform
// and decided on broadcast values:
//   LLL      lll_loop of lgs_lll_loop.h -- the loop of lgs_lll_reduce itself -- from the k the
//            insertion left, until k reaches d;
//   advance  the next block of the tour, or the next tour, or the end of the call;
//   enum     the Schnorr-Euchner search of the projected block, then the insertion.
// In the search lane l owns level kb + l: its x, c, step state and the distance above it are
// registers, and its partial centre sums S[l][j] = sum over the levels kb + j .. e of mu x are a
// row of an LDS stack.  The definition sums a centre from the block's last level downwards, so
// S[l][j] depends on the coefficients above level kb + j alone: when x of a level changes, every
// lane below extends its own sum by one multiply and one add, and a descent reads a centre that
// has seen exactly the operations of the definition's loop, in its order.  A node costs a
// constant number of wave operations whatever the block size.
// A launch advances a basis by at most l.slice LLL iterations and node_slice nodes; a basis
// suspended anywhere writes its complete state, the LDS image, back to its block.
#include <hip/hip_runtime.h>

#include <cmath>

#include "lgs_kernels.h"
#include "lgs_lll_loop.h"

namespace lgs {
namespace {

enum { kPhLll = 0, kPhAdvance = 1, kPhEnum = 2 };
// words of the header
enum { kHPhase = 0, kHKb, kHTours, kHIns, kHBlocks, kHInsertions, kHNodes, kHTruncated, kHNodesB, kHLevel, kHTop,
       kHA, kHBest };

// A value every lane holds, in scalar registers.
__device__ inline int64_t bkz_uni(int64_t v) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(v & 0xffffffff));
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(kLllLanes) void bkz_reduce_kernel(const BkzArgs a) {
    extern __shared__ int64_t lds[];
    const int d = a.l.d, ld = lll_ld(d), lane = threadIdx.x;
    const int64_t q = a.l.live_in ? a.l.live_in[blockIdx.x] : (int64_t)blockIdx.x;
    const size_t words = bkz_state_words(d);
    const LllLds s = lll_lds(lds, d);
    int64_t* bh = lds + lll_state_words(d);
    double* ex = (double*)(bh + kBkzHdr);
    double* ec = ex + kBkzLanes;
    double* eP = ec + kBkzLanes;
    double* estp = eP + kBkzLanes;
    double* enxt = estp + kBkzLanes;
    double* eS = enxt + kBkzLanes;
    double* ebest = eS + kBkzMaxBlock * kBkzSPitch;
    int64_t* st = a.l.state + (size_t)q * words;
    for (size_t w = lane; w < words; w += kLllLanes) lds[w] = st[w];
    __syncthreads();
    LllRun w;
    w.k = (int)bkz_uni(s.hdr[0]);
    w.iters = bkz_uni(s.hdr[1]);
    w.swaps = bkz_uni(s.hdr[2]);
    w.passes = bkz_uni(s.hdr[3]);
    w.status = (int)bkz_uni(s.hdr[4]);
    w.rd = s.rdiag[lane];  // r[lane][lane]
    int phase = (int)bkz_uni(bh[kHPhase]), kb = (int)bkz_uni(bh[kHKb]);
    int64_t tours = bkz_uni(bh[kHTours]), ins = bkz_uni(bh[kHIns]), blocks = bkz_uni(bh[kHBlocks]);
    int64_t insertions = bkz_uni(bh[kHInsertions]), nodes = bkz_uni(bh[kHNodes]);
    int64_t truncated = bkz_uni(bh[kHTruncated]), nodes_b = bkz_uni(bh[kHNodesB]);
    int li = (int)bkz_uni(bh[kHLevel]), top = (int)bkz_uni(bh[kHTop]);
    double A = __longlong_as_double(bkz_uni(bh[kHA]));
    int have_best = (int)bkz_uni(bh[kHBest]);
    const bool act = lane < d;
    int64_t budget = a.l.slice, nbudget = a.node_slice;
    while (w.status < 0) {
        if (phase == kPhLll) {
            lll_loop(s, d, lane, a.l.delta, a.l.eta, a.l.max_iters, budget, w);
            if (w.status != 0) break;  // out of iterations for this launch (-1), or stopped
            w.status = -1;
            phase = kPhAdvance;
        }
        if (phase == kPhAdvance) {
            if (tours == 0 || kb + 1 > d - 2) {
                if (tours > 0 && ins == 0) {
                    w.status = 0;
                    break;
                }
                if (tours == a.max_tours) {
                    w.status = 4;
                    break;
                }
                ++tours;
                ins = 0;
                kb = 0;
            } else {
                ++kb;
            }
            // ENUM(kb, e) starts: x = c = P = 0, every partial sum +0.0, the first node is the
            // zero vector on level kb
            ex[lane] = 0.0;
            ec[lane] = 0.0;
            eP[lane] = 0.0;
            estp[lane] = 1.0;
            enxt[lane] = 0.0;
            if (lane < kBkzMaxBlock)
                for (int j = 0; j < kBkzSPitch; ++j) eS[lane * kBkzSPitch + j] = 0.0;
            A = a.l.delta * lll_bcast(w.rd, kb);
            li = 0;
            top = 0;
            nodes_b = 0;
            have_best = 0;
            phase = kPhEnum;
        }
        // phase == kPhEnum: lane l works on level kb + l
        const int e = (kb + a.block_size < d ? kb + a.block_size : d) - 1;
        const int nl = e - kb + 1;
        const double rl = __shfl(w.rd, kb + lane < kLllLanes ? kb + lane : kLllLanes - 1);
        double x = ex[lane], c = ec[lane], P = eP[lane], stp = estp[lane], nxt = enxt[lane];
        double* Srow = eS + (lane < kBkzMaxBlock ? lane : kBkzMaxBlock - 1) * kBkzSPitch;
        const double* mul = s.mu + kb * ld + kb + (lane < kBkzMaxBlock ? lane : 0);  // mu[kb + j][kb + l] at j*ld
        int trunc = 0;
        bool finished = false;
        for (;;) {
            if (nodes_b == a.enum_nodes) {
                trunc = 1;
                finished = true;
                break;
            }
            if (nbudget == 0) break;
            --nbudget;
            ++nodes_b;
            ++nodes;
            double t = x - c;
            t = t * t;
            t = t * rl;
            const double Pi = lll_bcast(P + t, li);
            if (Pi < A) {
                if (li > 0) {  // descend, enter(li - 1): the centre is the lane's finished sum
                    if (lane == li - 1) P = Pi;
                    --li;
                    const double ci = lll_bcast(0.0 - Srow[li + 1], li);
                    if (!(fabs(ci) < kLllMaxX)) {
                        w.status = 2;
                        break;
                    }
                    const double xi = rint(ci);
                    if (lane == li) {
                        c = ci;
                        x = xi;
                        stp = ci >= xi ? 1.0 : -1.0;
                        nxt = 0.0;
                    }
                    if (lane < li) Srow[li] = Srow[li + 1] + mul[li * ld] * xi;
                    continue;
                }
                if (nodes_b != 1) {  // a vector of the block below the radius (not the zero vector)
                    A = Pi;
                    have_best = 1;
                    if (lane < nl) ebest[lane] = x;
                }
            } else {
                ++li;
                if (li >= nl) {
                    finished = true;
                    break;
                }
                if (li > top) top = li;
            }
            // the next sibling on level li: upwards only on the top level, zigzag below it
            if (lane == li) {
                if (li == top) {
                    x = x + 1.0;
                } else {
                    nxt = nxt + 1.0;
                    x = x + stp * nxt;
                    stp = -stp;
                }
            }
            const double xi = lll_bcast(x, li);
            if (lane < li) Srow[li] = Srow[li + 1] + mul[li * ld] * xi;
        }
        if (!finished) {  // suspended inside the enumeration, or stopped by its guard
            ex[lane] = x;
            ec[lane] = c;
            eP[lane] = P;
            estp[lane] = stp;
            enxt[lane] = nxt;
            break;
        }
        ++blocks;
        truncated += trunc;
        phase = kPhAdvance;
        if (!have_best) continue;
        // INSERT(kb, e, best): Euclid on the coefficients; lane c owns coordinate c of b and of U
        __syncthreads();
        int64_t carry = bkz_uni((int64_t)ebest[nl - 1]);
        for (int j = e; j > kb && w.status < 0; --j) {
            const int i = j - 1;
            int64_t xj = carry, xi = bkz_uni((int64_t)ebest[i - kb]);
            while (xj != 0) {
                const int64_t qq = xi / xj;
                int64_t bi = 0, ui = 0, nb = 0, nu = 0;
                if (act) {
                    bi = s.b[i * ld + lane];
                    ui = s.U[i * ld + lane];
                    nb = s.b[j * ld + lane] + qq * bi;
                    nu = s.U[j * ld + lane] + qq * ui;
                }
                const bool over = nb >= kLllMaxB || nb <= -kLllMaxB || nu >= kLllMaxU || nu <= -kLllMaxU;
                if (__any(over)) {  // the state before this step is the result
                    w.status = 2;
                    break;
                }
                if (act) {  // b_j += q b_i, then the swap
                    s.b[j * ld + lane] = bi;
                    s.b[i * ld + lane] = nb;
                    s.U[j * ld + lane] = ui;
                    s.U[i * ld + lane] = nu;
                }
                const int64_t rem = xi - qq * xj;
                xi = xj;
                xj = rem;
            }
            carry = xi;
        }
        __syncthreads();
        if (w.status >= 0) break;
        for (int k = kb; k <= e; ++k)  // rows and columns kb..e of G from b, exactly; lane j owns G[k][j]
            if (act) {
                int64_t g = 0;
#pragma unroll 4
                for (int cc = 0; cc < d; ++cc) g += s.b[k * ld + cc] * s.b[lane * ld + cc];
                s.G[k * ld + lane] = g;
                s.G[lane * ld + k] = g;
            }
        __syncthreads();
        ++insertions;
        ++ins;
        if (kb == 0) {  // r[0][0] of the vector that moved to the front
            const double r00 = (double)s.G[0];
            if (lane == 0) w.rd = r00;
            if (!lll_good(r00)) {
                w.status = 3;
                break;
            }
        }
        w.k = kb > 1 ? kb : 1;
        phase = kPhLll;
    }
    __syncthreads();
    if (w.status < 0) {  // suspended: the state back to its block, the basis onto the live list
        s.rdiag[lane] = w.rd;
        if (lane == 0) {
            s.hdr[0] = w.k;
            s.hdr[1] = w.iters;
            s.hdr[2] = w.swaps;
            s.hdr[3] = w.passes;
            s.hdr[4] = w.status;
            bh[kHPhase] = phase;
            bh[kHKb] = kb;
            bh[kHTours] = tours;
            bh[kHIns] = ins;
            bh[kHBlocks] = blocks;
            bh[kHInsertions] = insertions;
            bh[kHNodes] = nodes;
            bh[kHTruncated] = truncated;
            bh[kHNodesB] = nodes_b;
            bh[kHLevel] = li;
            bh[kHTop] = top;
            bh[kHA] = __double_as_longlong(A);
            bh[kHBest] = have_best;
            const unsigned long long at = atomicAdd(a.l.ctl, 1ull);
            if (at < (unsigned long long)a.l.nlive) a.l.live_out[at] = (int32_t)q;
        }
        __syncthreads();
        for (size_t v = lane; v < words; v += kLllLanes) st[v] = lds[v];
        return;
    }
    // stopped: the outputs in the caller's layout (vector i in column i)
    int64_t* bo = a.l.basis_out + (size_t)q * d * d;
    int64_t* uo = a.l.U_out + (size_t)q * d * d;
    if (act) {
        for (int cc = 0; cc < d; ++cc) {
            bo[(size_t)cc * d + lane] = s.b[lane * ld + cc];
            uo[(size_t)cc * d + lane] = s.U[lane * ld + cc];
        }
        if (a.l.gs_norm2) a.l.gs_norm2[(size_t)q * d + lane] = w.rd;
    }
    if (lane == 0) {
        if (a.l.swaps) a.l.swaps[q] = w.swaps;
        if (a.l.iters) a.l.iters[q] = w.iters;
        if (a.l.passes) a.l.passes[q] = w.passes;
        if (a.l.status) a.l.status[q] = w.status;
        if (a.tours) a.tours[q] = tours;
        if (a.blocks) a.blocks[q] = blocks;
        if (a.insertions) a.insertions[q] = insertions;
        if (a.nodes) a.nodes[q] = nodes;
        if (a.truncated) a.truncated[q] = truncated;
    }
}

}  // namespace

namespace launch {

hipError_t bkz_reduce(const BkzArgs& a, hipStream_t st) {
    const LllArgs& l = a.l;
    if (l.nlive <= 0) return hipSuccess;
    if (l.d < 2 || l.d > kLllMaxD || l.m < 1 || !l.state || l.nlive > l.m || !l.live_out || !l.ctl || !l.basis_out ||
        !l.U_out || l.slice < 1 || l.max_iters < 1 || a.node_slice < 1 || a.block_size < 2 ||
        a.block_size > kBkzMaxBlock || a.max_tours < 1 || a.enum_nodes < 1)
        return hipErrorInvalidValue;
    const size_t lds = bkz_lds_bytes(l.d);
    if (lds > 48 * 1024) {
        const hipError_t e =
            hipFuncSetAttribute((const void*)bkz_reduce_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(bkz_reduce_kernel, dim3((unsigned)l.nlive), dim3(kLllLanes), lds, st, a);
    return hipGetLastError();
}

}  // namespace launch
}  // namespace lgs
