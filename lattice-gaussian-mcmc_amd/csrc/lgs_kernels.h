// lgs_kernels.h -- internal interface between the C-ABI (lgs_capi.hip) and the
// kernels (lgs_kernels.hip).  Not part of the public ABI (see include/lgs.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Compile-time switches (-D) the sources still read; everything else is fixed.  The
// variants that were tried and removed are listed in DESIGN.md ("Variants tried and
// removed").
//   LGS_TEST_HOOKS    the hooks library: test and A/B switches read from the environment
//                     (Makefile; the tests that perturb the certificate load it)
//   LGS_NO_SPEC       no speculative sub-panels in klein_mfma_kernel
//                     (tests/test_gpu_certificate.py, tools/gpu_spec_check.sh)
//   LGS_OZ_DIGITS     R digits of the int8-digit far field, default 6 (tools/gpu_oz_digits.sh)
//   LGS_DIAG_CYCLES   per-phase shader-clock counters of klein_mfma_kernel (tools/kbench.py)
//   LGS_DIAG_FAR      per-wave shader-clock phases of the far field's chunk loop (tools/kbench.py)
//   LGS_DIAG_CAPQ     why the capped kind's quantile decision falls through (tools/kbench.py)

namespace lgs {

constexpr unsigned int kFlagNonFinite = 1u;  // a conditional mean was NaN/inf
constexpr unsigned int kFlagOverflow = 2u;   // |z| >= 2^31 with an int32 store
constexpr unsigned int kFlagI8Range = 4u;    // |z| > 32639: int8-digit B z must be redone in fp64
constexpr unsigned int kFlagOverflow16 = 8u; // |z| > 32767 in a 16-bit internal store
constexpr unsigned int kFlagCarry16 = 16u;   // a chain state carried into a 16-bit store does not fit
// lgs_imhk enqueues a block's Klein launch and its dependants without waiting: the
// dependants that modify caller state (acceptance, moments, state gathers, initial
// draws) return immediately when the launch set one of these, and the block is
// redone at the wider width after the call's single synchronisation
constexpr unsigned int kAbortMask = kFlagOverflow16 | kFlagCarry16;
// flags[1] of a launch: coordinates whose decision at the blocked-order mean could
// not be certified and was redone at the reference-order mean (lgs_device.h)
constexpr int kFlagWordResolved = 1;
constexpr int kFlagWordUninit = 4;      // lgs_imhk: some chain needs its initial draw
constexpr int kFlagWordCheckpoint = 5;  // lgs_imhk: resolved count before the block's Klein launch

constexpr int kErfTabLast = 512;
constexpr int kCoefStride = 18;  // doubles per grid point of the coefficient table (lgs_device.h CoefTab)  // SampleZ erf/exp table: y_j = j/64, j = 0..kErfTabLast (y <= 8)

// Per-coordinate SampleZ constants (kSzcStride doubles per coordinate, built by
// the host in lgs_set_basis; lgs_device.h sample_z_coord):
//   [0] sigma_i  [1] 1/sigma_i  [2] kind  [3] sc = sigma*sqrt(pi/2)  [4] 1/sc
//   [5] sigma*sqrt(2)  [6] rf*sigma (window half-width, klein.py:113-120)
//   [7] S, [8] base (kind kSzClosed); [7] of the capped kind: 1 when sigma >= 360
//   (series erf / exp over the whole window, lgs_device.h PolyErf)
//   [kSzS..kSzS+kSzDeg] / [kSzB..kSzB+kSzDeg]: monomial coefficients in
//   m = mu - rint(mu) of S(m) / base(m) (kind kSzCapped)
//   [kSzCa], [kSzCb]: decision certificate of the blocked kernels (lgs_device.h
//   certified decisions): |mu_fast - mu_ref| <= Ca + Cb * sum_{j>i} |z_j| + 6e-16 |mu|
//   [7] of the small kind: 1 when points entering / leaving the window at its ends
//   can carry more than 2^-60 of the mass (the certificate then checks the ends)
constexpr int kSzDeg = 5;  // degree 4 already reaches the fp64 floor for sigma in [50, 1e6]
constexpr int kSzS = 9;
constexpr int kSzB = kSzS + kSzDeg + 1;
constexpr int kSzCa = kSzB + kSzDeg + 1;  // 21
constexpr int kSzCb = kSzCa + 1;
constexpr int kSzUsed = kSzCb + 1;  // 23
constexpr int kSzcStride = 24;
// Klein-path record per coordinate (kRecStride doubles): the SampleZ constants
// [0, kSzUsed), then c', 1/R_ii, the dispatch code, R_ii/sigma, 1/sigma_i^ref, lterm,
// CbC, and the 15 near-field coefficients R[i-1-m][i] of the coordinate's 16-row
// sub-panel.  Staged into LDS once per 32-row panel by klein_mfma_kernel.
// The dispatch code and the weight constants come before the near-field
// coefficients: the step's decision then waits for the first 15 of the record's 22
// 16-byte reads, and Rs[1..14] arrive while it runs.  Round 6, measured together with
// the record's LDS reads left to the scheduler (load_rec) and the Philox round keys left
// to loop-invariant motion (philox4x32_10), identical outputs; each alone is within
// noise, together the bench 117.0-117.4 -> 118.9-119.6 M samples/s and Klein 28.84-28.93
// -> 28.20-28.34 ms per 2^22 block (profiles/r06au_bench_variants.log), C3 / C4 / C5
// Klein -1.6 / -1.0 / -1.3 % at 2^20 samples and C1 / C2 +1.7 / +1.2 %
// (r06av_call_kbench.log).
//   kRecDisp   SampleZ dispatch code of the coordinate (host): 0.0 = small kind with one
//              dominant window point possible (q[7] == 0), 1.0 = capped kind with
//              sigma >= 360 (q[7] == 1), 2.0 = anything else (sigma_i == 0 included)
//   kRecCbC    Cb of the certificate for a mean whose far field used only the 3 most
//              significant R digits (reference mode, panels of two speculative
//              sub-panels: klein_mfma_kernel)
constexpr int kRecCp = kSzUsed, kRecIrii = kSzUsed + 1, kRecDisp = kSzUsed + 2, kRecRos = kSzUsed + 3,
              kRecIsr = kSzUsed + 4, kRecLterm = kSzUsed + 5, kRecCbC = kSzUsed + 6, kRecRs = kSzUsed + 7;
// int8-digit far field (klein_mfma_kernel OZ): row scale 2^E_i of the
// coordinate's row over its panel's far columns
constexpr int kRecScale = kRecRs + 15;
// 1.0 when the coordinate's 16-row sub-panel is whole and all its coordinates are
// of the small kind with one dominant window point possible (q[7] == 0): the
// sub-panel is then decided speculatively in parallel (klein_mfma_kernel)
constexpr int kRecSpec = kRecScale + 1;
constexpr int kRecStride = 48;  // 384 bytes, 16-byte multiple
// B z (bz_i8_kernel): coordinates per workgroup tile (64 was tried: half the
// accumulators per wave, twice the workgroups)
constexpr int kBzBN = 128;
// words per 128-row tile of B in the off-diagonal table (one bit per 64-coordinate chunk,
// d <= kOzMaxD = 32768)
constexpr int kBzOffdWords = 32768 / 64 / 32;
// bz_lean_kernel: unused LDS bytes added to each workgroup's 17 408, so that three fit a
// 160 KB CU.  The kernel runs beside the next block's Klein launch, on the CUs kept free
// for it and in whatever a retiring Klein workgroup frees; at the 8 workgroups per CU its
// 40 VGPRs allow it crowds those slots and delays the Klein launch's own workgroups (C3
// bench 35.6 ms per step against the parent's 32.9; 5 per CU 34.7, 2 per CU 32.8, 3 per
// CU 31.5: profiles/r08b_lean_ab.log).
constexpr int kBzLeanPadLds = 36000;
static_assert(kRecCbC < kRecStride, "record layout");
constexpr int kOzCoarse = 4;  // R digits of the far field in coarse panels
// int8-digit far field layout: per 32-row panel pk >= 1 (K = 32 pk far columns,
// ceil(K/64) chunks of 64): [chunk][row tile t][digit a][lane][16 bytes]
#ifndef LGS_OZ_DIGITS
#define LGS_OZ_DIGITS 6
#endif
constexpr int kOzDigits = LGS_OZ_DIGITS;  // R digits: 48 significant bits (the rounding adds 128 u M to Cb, lgs_set_basis)
constexpr int kOzMaxD = 32768;  // int32 class sums stay exact: 2 * K * 2^14 < 2^31
constexpr int kSzRound = 0;    // sigma_i < 1e-10: round(mu), no draw
constexpr int kSzSmall = 1;    // sigma_i < 4: <= 4-point exponent path / table walk
constexpr int kSzClosed = 2;   // uncapped window of +-rf*sigma, rf >= 9: S = 2 sc, base = -sc
constexpr int kSzCapped = 3;   // window capped to rint(mu) +- 500: S(m), base(m) polynomials
constexpr int kSzGeneric = 4;  // anything else: both window ends evaluated per draw

constexpr int kKernelExact = 0;  // reference-order back-substitution
constexpr int kKernelValu = 1;   // blocked panel kernel, VALU far field
constexpr int kKernelMfma = 2;   // blocked panel kernel, fp64 MFMA far field

// Per-launch arguments of the Klein samplers.  Per-coordinate arrays (length d):
//   cp      c' = Q^T c
//   rii     R_ii (> 0 after the sign fix of klein.py:69-73)
//   sig     effective SampleZ sigma: sigma/R_ii, clamped to 1e6 above 1e10,
//           0 when sigma/R_ii < 1e-10 (deterministic rounding)
//   sig_ref sigma/R_ii unclamped (reference-mode weight, klein.py:255-263)
//   lterm   0.5*log(2*pi) + log(sig_ref)
//   irii    1/R_ii, ros = R_ii/sigma, isr = 1/sig_ref (reciprocal forms for the
//           fast kernels; the exact-order kernel divides like the reference)
struct KleinArgs {
    int d;
    int precision;
    int linear_probs;
    int counter_mode;  // 0: lane p -> sample base+p; 1: chain0 + p/nt, step0 + p%nt (chain-major)
    const double* cp;
    const double* rii;
    const double* sig;
    const double* sig_ref;
    const double* lterm;
    const double* irii;
    const double* ros;
    const double* isr;
    const double* R;     // row-major R (reference-order means of uncertified decisions)
    double sigma;
    double z1cap;        // 32-row panels: certificate bound on sum_j |z_j| (verified per sub-panel)
    unsigned long long* z1max;  // 32-row panels: atomicMax of the samples' sum |z_j| (fp64 bits)
    uint64_t seed;
    uint64_t base;
    uint32_t chain0;
    uint32_t step0;
    int64_t nt;
    int64_t n;
    int64_t ldz;
    double* LW;
    unsigned int* flags;
    const double* etab;  // SampleZ erf/exp table (nullptr: ocml libm path)
    const double* etab2; // its Taylor-coefficient form (lgs_device.h CoefTab)
    const double* szc;   // per-coordinate SampleZ constants (nullptr: generic sample_z)
    const double* cert;  // per coordinate {Ca, Cb} of the decision certificate (kSzCa / kSzCb)
    const double* crec;  // per-coordinate records (kRecStride doubles, layout above)
    // int8-digit far field (nullptr rd: fp64 MFMA far field)
    const int8_t* rd;        // R digit fragments, all panels
    const int64_t* rd_off;   // byte offset of panel pk in rd
    int16_t* h16;            // coefficient history, [(i + h16_shift)/16][lane][16] int16
    int h16_shift;           // (16 - d % 16) % 16
    int64_t h16_lanes;       // lanes per 16-coordinate block (>= n)
    uint8_t* znz;            // nullable (with h16): [(i + h16_shift)/16][lane] 1 when the lane's z of
                             // that block has a nonzero (B z skips chunks that are all zero)
    const double* rx;    // per 32-row panel: 16x16 block R[p_hi-32.., p_hi-16..] as MFMA A fragments
    const unsigned int* gate;  // nullable: when *gate == 0 every block returns at once (initial draws
                               // of lgs_imhk when no chain needs one, decided on the device)
    // Wang-Ling mode, blocked kernels (nullable): per sample a bound E >= |LW - LW_ref|,
    // LW_ref = the log weight at the reference-order means (what klein_exact_kernel
    // returns), from the certificate's bound on each mean (lgs_kernels.hip wl_bound_*)
    double* LWE;
    unsigned long long* emax;  // nullable: atomicMax of those bounds (fp64 bits, E >= 0)
    // q-panel skip (reference mode, int8-digit far field; nullable): per 32-row panel the
    // largest ||z_W||^2 for which every row's mean is certified to give z = 0 without
    // computing it (lgs_set_basis), < 0 where it does not apply
    const double* qz2;
    // nullable (with h16, d % 16 == 0): per wave of the launch, bit c & 31 of word
    // clive[(c >> 5) * clive_ld + wave] set when some lane has a nonzero z in the
    // 64-coordinate chunk c (zeroed before the launch; B z's chunk skipping)
    unsigned int* clive;
    int64_t clive_ld;
    // q-panel skip, clean state (nullable; with qz2 and h16, at most kQCleanPanels 32-row
    // panels; a multiple of 4 bytes, 4-byte aligned): byte qclean[wave * npan + pk], wave
    // = p / 64 of the launch, nonzero when that wave's Z rows, history blocks and znz
    // bytes of panel pk hold the skip's values (0, z + 128 = 0x0080, 0) since its last
    // launch into the same buffers.  A wave that skips such a panel stores nothing.
    // Each byte is read and written only by the wave that owns it.  qclean_reset != 0:
    // the bytes are not read (every panel counts as dirty) and all are rewritten;
    // qclean_gate (nullable): the same when *qclean_gate != 0 (the device word that
    // gated a launch into the store since: lgs_imhk's initial draws).
    uint8_t* qclean;
    int qclean_reset;
    const unsigned int* qclean_gate;
};
constexpr int kQCleanPanels = 128;  // d <= 4096

// Counter / check words of the context's flag buffer used by the certified
// Wang-Ling accept decisions (imhk_accept_kernel)
constexpr int kFlagWordAcceptResolved = 6;  // decisions redone at reference-order weights
constexpr int kFlagWordWLMismatch = 7;      // recomputed draws that did not reproduce the stored z (a bug)
constexpr int kFlagWordQSkip = 8;           // (wave, panel) pairs of the q-panel skip (klein_mfma_kernel)
constexpr int kFlagWordDecodeResolved = 9;  // lgs_klein_decode: targets whose winner the bounds did not decide
constexpr int kFlagWordQSkipElided = 10;    // those whose stores were elided (KleinArgs::qclean)
constexpr int kFlagWords = 16;             // the flag buffer: 64 bytes

// Per-lane outputs of the decode sampling kernels (lgs_klein_decode): K draws per
// target, lane p = t K + k; D[p] the draw's squared distance to its target as the kernel
// formed it, E[p] >= |D[p] - reference-order distance|.
struct DecodeLanes {
    int64_t K;
    double* D;
    double* E;
};

// The sampling kernels of lgs_imhk_targets: K = n_steps + 1 draws per target, lane
// p = k K + t (counter_mode 1, nt = K).  The lanes' Wang-Ling log weights and their
// bounds go to KleinArgs::LW / LWE (both non-null).
struct WeightLanes {
    int64_t K;
};

// The Metropolis scan of lgs_imhk_targets (imhk_targets_accept_kernel): chain k < nc
// owns the draws of columns k K .. k K + K - 1, draw 0 its initial state.
struct ImhkTargetsArgs {
    int64_t nc;
    int64_t K;
    uint64_t seed;
    uint32_t chain0;
    double* LW;             // per draw: log weight (recomputed ones are written back)
    double* LWE;            // per draw: E >= |LW - reference-order log weight| (then 0)
    const double* RT;       // R transposed, d x d
    const void* Zst;        // the draws (coordinate-major, column p, ld ldz, zb-byte elements)
    int zb;
    int64_t ldz;
    const double* CP;       // the chains' centres, coordinate-major: CP[i * ldc + k]
    int64_t ldc;
    int64_t* final_col;     // nc: the column of the chain's final state
    double* logw;           // nullable, nc: its log weight
    int64_t* accepts;       // nullable, nc: accepted proposals (overwritten)
    int64_t* final_step;    // nullable, nc: its counter step
    uint8_t* accepted;      // nullable, nc x (K - 1)
    unsigned int* flagw;    // the context's flag words (kFlagWordAcceptResolved, kFlagWordWLMismatch)
    double bscale;          // bounds x bscale (1; a test hook widens them to force recomputations)
};

// ---- exact closest vector: Schnorr-Euchner enumeration (lgs_cvp.hip, lgs_closest_vector)
constexpr int kCvpMaxD = 64;               // LGS_CVP_MAX_D: R fits 32 KB of LDS
constexpr int64_t kCvpSlice = 1 << 16;     // tree nodes a lane visits per launch at most
constexpr int64_t kCvpMaxSlots = 1 << 16;  // lanes of one launch (the state block's columns)
constexpr int kCvpLanes = 64;              // lanes of a block: one wave
constexpr double kCvpMaxAbsZ = 4503599627370496.0;  // 2^52: a conditional mean at or beyond it is an error
// LDS of a block: R, then base | P | z | sn of its lanes (lgs_cvp.hip)
inline size_t cvp_lds_bytes(int d) { return ((size_t)d * d + (size_t)4 * d * kCvpLanes) * 8; }
// The search state of one slot (= lane): element (i, s) of a per-level array at
// [i * S + s], S the slot count of the block, so the lanes of a wave that stand on the same
// level read adjacent addresses.  It persists between launches: a launch loads the scalars,
// advances the search by at most `slice` nodes and stores them back.
struct CvpState {
    double* z;       // d x S: the current point's coefficients (integers, |z| < 2^53)
    double* base;    // d x S: c'_i - cs of the level's entry
    double* P;       // d x S: partial distance of levels >= i (row 0 unused, P[d] = 0 implied)
    double* sn;      // d x S: stp * (nxt + 1), the zig-zag's next offset with its sign (an integer)
    int64_t* best;   // d x S: the best point found
    double* A;       // S: the bound (radius2, then the best point's distance)
    int64_t* nodes;  // S: nodes visited for the slot's target
    int32_t* tgt;    // S: the chunk's target the slot works on, -1 = idle
    int32_t* lvl;    // S: the level i
    int32_t* has_best;  // S
};
inline size_t cvp_state_bytes(int d, int64_t S) { return (size_t)S * ((size_t)d * 40 + 28); }
inline CvpState cvp_state_at(void* p, int d, int64_t S) {  // (S a multiple of 64: every array 8-byte aligned)
    CvpState s;
    const size_t n = (size_t)d * S;
    s.z = (double*)p;
    s.base = s.z + n;
    s.P = s.base + n;
    s.sn = s.P + n;
    s.best = (int64_t*)(s.sn + n);
    s.A = (double*)(s.best + n);
    s.nodes = (int64_t*)(s.A + S);
    s.tgt = (int32_t*)(s.nodes + S);
    s.lvl = s.tgt + S;
    s.has_best = s.lvl + S;
    return s;
}
struct CvpArgs {
    int d;
    int64_t m;          // targets of the chunk
    int64_t nslots;     // lanes of this launch (slots [0, nslots) of the block)
    int64_t S;          // the state block's slot count
    int64_t max_nodes;  // per target
    int64_t slice;      // per lane and launch
    const double* R;    // row-major d x d
    const double* CP;   // the targets' centres, coordinate-major: CP[i * ldc + t]
    int64_t ldc;
    const double* radius2;  // nullable, m
    CvpState st;
    // ctl[0]: the next target to hand out (an idle lane takes it; >= m: none left);
    // ctl[1]: slots still working on a target when the launch ended (zeroed before it)
    unsigned long long* ctl;
    void* W;            // the returned points, coordinate-major, ld ldw, 4- or 8-byte elements
    int64_t ldw;
    double* dist2;      // m
    int64_t* nodes;     // m
    int32_t* status;    // m
    unsigned int* flags;  // the context's flag words (kFlagNonFinite, kFlagOverflow)
};

// ---- exact closest vector over a batch of bases (lgs_cvpb.hip, lgs_closest_vector_bases;
// DESIGN.md 6k).  One basis per block of one wave, problem (p, k) -- target k of basis p --
// on lane k.  Slot q of the chunk's workspace holds basis off + q:
//   R        m x d x d row-major: the factor (zeros for a refused basis)
//   CP       m x d x kCvpLanes: c' the way the enumeration reads it, CP[(q d + i) 64 + k]
//   cprime   m x T x d: the same numbers in the caller's layout
//   st       a CvpState of S = 64 m slots, problem (q, k) in slot 64 q + k; tgt is the
//            problem's phase (kCvpbFresh / kCvpbRunning / kCvpbDone)
//   pstatus  64 m: the status of a done problem (0 / 1 / 2; 3 = its basis was refused)
constexpr int kCvpbMaxT = 64;             // LGS_CVPB_MAX_T: a wave's lanes
constexpr int64_t kCvpbSlice = 1 << 16;   // tree nodes a problem advances per launch at most
constexpr int64_t kCvpbSlots = 1024;      // bases of one chunk (338 MB of workspace at d = T = 64)
constexpr int kCvpbFresh = 0, kCvpbRunning = 1, kCvpbDone = 2;
__host__ __device__ inline int cvpb_ld(int d, int T) { return (d + T) | 1; }  // W's row pitch in LDS
inline size_t cvpb_qr_lds_bytes(int d, int T) { return (size_t)d * cvpb_ld(d, T) * 8; }  // 66 048 B at d = T = 64
struct CvpbArgs {
    int d, T;
    int64_t m;             // bases of the chunk
    int64_t nlive;         // (cvpb_enum) blocks of this launch
    int64_t max_nodes, slice;
    const double* bases;   // m x d x d (the caller's or the staged copy)
    const double* targets; // m x T x d
    const double* radius2; // nullable, m x T
    double* R;
    double* CP;
    double* cprime;
    int32_t* qr_status;    // m
    int64_t S;             // the state block's slot count (>= 64 m)
    CvpState st;
    int32_t* pstatus;
    const int32_t* live_in;  // (cvpb_enum) nullable: the bases of this launch (none: 0 .. nlive-1)
    int32_t* live_out;       // the bases with an unfinished problem, ctl[0] of them
    unsigned long long* ctl;
    unsigned int* flags;     // one word: kFlagNonFinite, kFlagOverflow
    // cvpb_finish: the chunk's outputs, in the caller's layout
    void* z;        // m x T x d, zb-byte elements
    double* v;      // m x T x d
    double* dist2;  // m x T
    int64_t* nodes;
    int32_t* status;
};

// ---- Klein draws over a batch of bases (lgs_kleinb.hip, lgs_klein_bases).
// The factor and the centres come from cvpb_qr (a CvpbArgs without CP, state block and
// pstatus).  Lane m of basis q is draw (k, j) = (m / K, m % K) of that basis; a block of
// kleinb_lanes(d) lanes belongs to one basis.  The chunk's workspace:
//   ZW   (m T K) x d, zb-byte elements: every draw, in the caller's layout
//   DW   m T K: the draws' reference-order distances
constexpr int kKleinbMaxT = 64;               // LGS_KLEINB_MAX_T
constexpr int64_t kKleinbSlots = 1024;        // bases of one chunk at most
constexpr int64_t kKleinbMaxDraws = 1 << 22;  // draws of one chunk at most (and T K of a call)
// Lanes of a block: the z image d x lanes x 8 B beside R has to leave room for a second block
// at d <= 32 (64 KiB of 160) and to fit at all at d = 64 (64 KiB at 128 lanes).
__host__ __device__ inline int kleinb_lanes(int d) { return d <= 32 ? 256 : 128; }
// The targets a block's lanes can touch: L consecutive lanes span at most this many m / K.
__host__ __device__ inline int kleinb_nt(int T, int64_t K, int L) {
    const int64_t span = (L + K - 2) / K + 1;
    return (int)(span < T ? span : T);
}
// LDS of a block, in doubles: R (d x d) | R_ii (d) | s_i (d) | c' (d x nt) | z (d x L)
inline size_t kleinb_lds_bytes(int d, int T, int64_t K) {
    const int L = kleinb_lanes(d);
    return ((size_t)d * d + 2 * (size_t)d + (size_t)d * kleinb_nt(T, K, L) + (size_t)d * L) * 8;
}
struct KleinbArgs {
    int d, T, zb, precision;
    int64_t K;             // draws per target
    int64_t m;             // bases of the chunk
    uint64_t seed, base;   // base: the Klein sample index of the chunk's draw (0, 0, 0)
    const double* bases;   // m x d x d (kleinb_select: v)
    const double* sigma;   // m
    const double* R;       // m x d x d
    const double* cprime;  // m x T x d
    const int32_t* qr_status;
    const double* etab;    // SampleZ table (nullptr: the libm path)
    void* ZW;
    double* DW;
    unsigned int* flags;   // one word: kFlagNonFinite, kFlagOverflow
    // kleinb_select: the chunk's per-problem outputs
    void* z;               // m x T x d, zb-byte elements
    double* v;             // m x T x d
    int64_t* best;         // m x T
    double* dist2;         // m x T
    int32_t* status;       // m x T
    // kleinb_draw_wl (lgs_imhk_bases): K = C S1 draws per target, lane m of a basis is draw
    // t = m % S1 of chain base + q T C + m / S1 (base: the chunk's first chain id), and DW holds
    // the draws' Wang-Ling log weights (a refused basis: -inf)
    int64_t S1;            // n_steps + 1
};

// ---- IMHK chains over a batch of bases (lgs_kleinb.hip, lgs_imhk_bases): the
// accept scan over the weights kleinb_draw_wl left in LW, and the gather out of its draws ZW.
// Chain g = (q T + k) C + j of the chunk owns draws g S1 .. g S1 + S1 - 1.
struct ImhkbArgs {
    int d, T, zb, thin;
    int64_t C, S1, m;       // chains per target, n_steps + 1, bases of the chunk
    int64_t n_keep;         // (S1 - 1) / thin
    uint64_t seed, base;    // base: the chunk's first chain id
    const double* bases;    // m x d x d
    const int32_t* qr_status;
    const double* LW;       // (m T C) x S1
    const void* ZW;         // (m T C S1) x d, zb-byte elements
    // imhkb_scan
    uint8_t* accepted;      // (m T C) x (S1 - 1)
    int64_t* accepts;       // m T C
    int64_t* final_step;    // m T C (-1 for a refused basis)
    double* logw;           // m T C
    int32_t* sel;           // (m T C) x n_keep: the state's draw after steps thin, 2 thin, .. (nullable)
    // imhkb_gather
    void* z;                // (m T C) x d
    double* v;              // (m T C) x d
    int32_t* status;        // m x T
    void* zs;               // (m T C n_keep) x d (nullable; needs sel)
};

// ---- LLL basis reduction (lgs_lll.hip, lgs_lll_reduce)
// One basis per block of one wave.  The block's LDS and the basis's state block in device
// memory have one layout, in 8-byte words, ld = lll_ld(d) (odd: a column sweep by 32 lanes
// touches 32 different 8-byte bank pairs):
//   b | U | G | mu   each d x ld: b[i*ld + c] coordinate c of vector i, U likewise (column i
//                    of the transform), G the int64 Gram matrix, mu the fp64 coefficients
//   rdiag            kLllLanes words: r[i][i] (0.0 where never computed)
//   header           kLllHdr words: k, iters, swaps, passes, status (-1 = still running)
// A launch loads the state, advances the basis by at most `slice` main-loop iterations and
// stores it back; a basis that stops writes its outputs instead and drops out of the live list.
constexpr int kLllMaxD = 64;            // LGS_LLL_MAX_D
constexpr int kLllLanes = 64;           // lanes of a block: one wave
constexpr int kLllHdr = 8;
constexpr int64_t kLllSlice = 1 << 12;  // main-loop iterations of a basis per launch at most
constexpr int64_t kLllChunk = 1024;     // bases of one state block (134 MB at d = 64)
constexpr int64_t kLllMaxB = (int64_t)1 << 28;  // |b| entries stay below it
constexpr int64_t kLllMaxU = (int64_t)1 << 40;  // |U| entries
constexpr double kLllMaxX = 4194304.0;          // 2^22: |X|
constexpr unsigned int kLllFlagRange = 1u;      // LllArgs::flags: an input |entry| >= 2^28
__host__ __device__ inline int lll_ld(int d) { return d | 1; }
__host__ __device__ inline size_t lll_state_words(int d) { return (size_t)4 * d * lll_ld(d) + kLllLanes + kLllHdr; }
inline size_t lll_lds_bytes(int d) { return lll_state_words(d) * 8; }  // 133 696 B at d = 64
struct LllArgs {
    int d;
    int64_t m;           // bases of the chunk
    int64_t nlive;       // blocks of this launch
    const int32_t* live_in;  // nlive basis numbers (nullptr: block q works on basis q)
    int32_t* live_out;   // the bases still running when the launch ends, in any order
    unsigned long long* ctl;  // ctl[0]: entries of live_out (zeroed before the launch)
    int64_t slice;       // main-loop iterations per basis and launch
    int64_t max_iters;
    double delta, eta;
    int64_t* state;      // m state blocks of lll_state_words(d) words
    size_t state_words;  // (lll_init) the pitch of the state blocks when it is not that: lgs_bkz_reduce's
    const int64_t* basis;  // m x d x d row-major, vector i in column i (lll_init only)
    int64_t* basis_out;  // m x d x d
    int64_t* U_out;      // m x d x d
    int64_t* swaps;      // m (each of the five nullable)
    int64_t* iters;
    int64_t* passes;
    int32_t* status;
    double* gs_norm2;    // m x d
    unsigned int* flags;  // one word: kLllFlagRange
};

// ---- BKZ basis reduction (lgs_bkz.hip, lgs_bkz_reduce)
// One basis per block of one wave, on the LLL image above extended by the state of the tour and
// of the block enumeration in work; as there, the state block in device memory is the LDS image:
//   LLL image        lll_state_words(d) words
//   header           kBkzHdr words: phase, kb, tours, ins, blocks, insertions, nodes, truncated,
//                    nodes_b, level i, top (both relative to kb), A (fp64), best exists
//   x | c | P | stp | nxt   kBkzLanes words each, fp64: lane l owns level kb + l; x, stp and nxt
//                    hold integers (exact in fp64), P is P[kb + l + 1], the distance above the level
//   S                kBkzMaxBlock x (kBkzMaxBlock + 1) fp64: S[l][j] the partial centre sum of
//                    level kb + l over the levels kb + j .. e (row pitch odd: a lane owns a row)
//   best             kBkzMaxBlock words, fp64: x[kb .. e] of the shortest vector found
// A launch advances a basis by at most `slice` LLL iterations and `node_slice` enumeration nodes.
constexpr int kBkzMaxBlock = 32;  // LGS_BKZ_MAX_BLOCK
constexpr int kBkzHdr = 16;
constexpr int kBkzLanes = 64;
constexpr int kBkzSPitch = kBkzMaxBlock + 1;
constexpr int64_t kBkzNodeSlice = 1 << 16;  // enumeration nodes of a basis per launch at most
constexpr int kBkzExtWords = kBkzHdr + 5 * kBkzLanes + kBkzMaxBlock * kBkzSPitch + kBkzMaxBlock;
__host__ __device__ inline size_t bkz_state_words(int d) { return lll_state_words(d) + kBkzExtWords; }
inline size_t bkz_lds_bytes(int d) { return bkz_state_words(d) * 8; }  // 145 088 B at d = 64
// what BKZ adds fits beside the largest LLL image in the 160 KiB of a CU
static_assert(kBkzExtWords * 8 <= 160 * 1024 - (4 * kLllMaxD * (kLllMaxD | 1) + kLllLanes + kLllHdr) * 8,
              "the BKZ state does not fit in LDS");
static_assert(kBkzExtWords * 8 <= 30144, "the BKZ state exceeds the LDS the LLL image leaves at d = 64");
struct BkzArgs {
    LllArgs l;            // state: m blocks of bkz_state_words(d) words; l.slice, l.max_iters, outputs
    int block_size;
    int64_t max_tours, enum_nodes;
    int64_t node_slice;   // enumeration nodes per basis and launch
    int64_t* tours;       // m (each of the five nullable)
    int64_t* blocks;
    int64_t* insertions;
    int64_t* nodes;
    int64_t* truncated;
};

// ---- exact Gaussian mass: fixed-radius enumeration (lgs_cvp.hip, lgs_gaussian_mass)
// The search of lgs_cvp.hip with a bound that never shrinks and a weight on every leaf.  A
// work item is a partial tree: (target, top, prefix) -- the lane starts on level top - 1
// below the node z[top .. d-1] with partial distance P[top], and stops when it climbs back
// to `top` (top = d: the whole tree, no prefix).  kCvpSlice, kCvpMaxSlots, kCvpLanes and
// kCvpMaxAbsZ hold here too.
constexpr int kMassMaxD = kCvpMaxD;     // LGS_MASS_MAX_D
constexpr int kMassMomentsMaxD = 40;    // LGS_MASS_MOMENTS_MAX_D: msub | S join base | P | z | sn in LDS
// LDS of a block: R, then base | P | z | sn (| msub | S with moments) of its lanes
inline size_t mass_lds_bytes(int d, bool moments) {
    return ((size_t)d * d + (size_t)(moments ? 6 : 4) * d * kCvpLanes) * 8;
}
// The state of one slot, CvpState's layout rules: element (i, s) at [i * S + s].
struct MassState {
    double* z;       // d x S
    double* base;    // d x S
    double* P;       // d x S (P[top] is the item's, levels above it unused)
    double* sn;      // d x S
    double* msub;    // d x S (moments): the weight below the current node of level i, 1 <= i < top
    double* Sz;      // d x S (moments): sum of weight * z_i over the subtrees left so far, i < top
    double* mass;    // S
    double* energy;  // S
    double* dmin;    // S
    int64_t* points; // S
    int64_t* nodes;  // S
    int32_t* item;   // S: the work item the slot is on, -1 = idle
    int32_t* lvl;    // S
};
inline size_t mass_state_bytes(int d, int64_t S, bool moments) {
    return (size_t)S * ((size_t)d * (moments ? 48 : 32) + 48);
}
inline MassState mass_state_at(void* p, int d, int64_t S, bool moments) {  // (S a multiple of 64)
    MassState s;
    const size_t n = (size_t)d * S;
    s.z = (double*)p;
    s.base = s.z + n;
    s.P = s.base + n;
    s.sn = s.P + n;
    s.msub = s.sn + n;
    s.Sz = s.msub + (moments ? n : 0);
    s.mass = s.Sz + (moments ? n : 0);
    s.energy = s.mass + S;
    s.dmin = s.energy + S;
    s.points = (int64_t*)(s.dmin + S);
    s.nodes = s.points + S;
    s.item = (int32_t*)(s.nodes + S);
    s.lvl = s.item + S;
    return s;
}
// The per-item results of one pass, on the device and in the host's copy: mass | energy | dmin
// | points | nodes | status of ldo items each, 44 bytes per item, then sz (moments: d x ldo).
// ldo is a multiple of 64, so every array is 8-aligned.
struct MassItemOut {
    double *mass, *energy, *dmin, *sz;
    int64_t *points, *nodes;
    int32_t* status;
};
inline size_t mass_out_bytes(int d, int64_t ldo, bool moments) {
    return (size_t)ldo * (44 + (moments ? (size_t)d * 8 : 0));
}
inline MassItemOut mass_out_at(void* p, int64_t ldo, bool moments) {
    MassItemOut o;
    o.mass = (double*)p;
    o.energy = o.mass + ldo;
    o.dmin = o.energy + ldo;
    o.points = (int64_t*)(o.dmin + ldo);
    o.nodes = o.points + ldo;
    o.status = (int32_t*)(o.nodes + ldo);
    o.sz = moments ? (double*)(o.status + ldo) : nullptr;
    return o;
}
struct MassArgs {
    int d;
    int top;             // the level the items hang from (d: whole trees)
    int64_t m;           // work items of the chunk
    int64_t nslots;      // lanes of this launch
    int64_t S;           // the state block's slot count
    int64_t max_nodes;   // per item
    int64_t slice;       // per lane and launch
    double two_s2;       // 2 sigma^2
    const double* R;     // row-major d x d
    const double* CP;    // the targets' centres, coordinate-major: CP[i * ldc + t]
    int64_t ldc;
    const double* radius2;  // per target
    const double* shift;    // per target, nullable (0)
    const int32_t* it_tgt;  // m: the item's target (nullptr: item q is target q)
    const double* it_z;     // (d - top) x ldi: z[top + r] of item q at [r * ldi + q]
    const double* it_P;     // m: P[top] (nullptr with top = d)
    int64_t ldi;
    MassState st;
    unsigned long long* ctl;  // as CvpArgs::ctl
    // per item: results (o_sz: d x ldo coordinate-major, rows top .. d-1 zero; moments only)
    double *o_mass, *o_energy, *o_dmin, *o_sz;
    int64_t *o_points, *o_nodes;
    int32_t* o_status;   // 0 = the item's tree is done, 1 = max_nodes reached, 2 = a non-finite mean
    int64_t ldo;
    unsigned int* flags;
    // the listing pass (mass_list; lgs_ball_points, lgs_exact_table): point number p of item q
    // (in the item's traversal order) becomes row it_first[q] + p of l_z (row-major, d elements
    // of l_zb bytes) and l_d; rows at or beyond l_rows are not written
    const int64_t* it_first;  // m
    void* l_z;
    double* l_d;
    int l_zb;                 // 4 or 8
    int64_t l_rows;
};

// ---- exact sampler: inverse-CDF draws from a listed ball (lgs_exact.hip; lgs_exact_table,
// lgs_exact_sample).  The table's rows of target t are off[t] .. off[t+1]-1; its blocks of
// kExactBlock consecutive rows restart at every target: target t owns blocks boff[t] ..
// boff[t+1]-1 of the call.
constexpr int kExactBlock = 256;
struct ExactTable {
    int64_t n;           // targets
    int64_t nblocks;     // boff[n]
    const int64_t* off;  // n + 1
    const int64_t* boff; // n + 1
    const double* D;     // rows
    double* W;           // rows: weights
    double* S;           // rows: c_m, then S_m
    double* btot;        // nblocks: c of the block's last row
    double* bpre;        // nblocks: P_b
    double* mass;        // n
};
struct ExactDrawArgs {
    int d;
    int64_t K;           // draws per target
    int64_t j0, m;       // the chunk: draws j0 .. j0 + m - 1 of the call (draw j: target j / K)
    uint64_t seed, first;
    const int64_t* off;
    const double *S, *D, *mass;
    const void* Z;       // the table's rows, row-major, tb-byte elements
    void* W;             // the chunk's coefficients, coordinate-major, ld ldw, ob-byte elements
    int64_t ldw;
    int64_t* index;      // m, nullable
    double* dist2;       // m, nullable
    unsigned int* flags;
};

struct AcceptArgs {
    int64_t nc;
    int64_t T;
    int64_t thin;
    int64_t n_keep;
    uint64_t seed;
    uint32_t chain0;
    uint32_t step0;
    const double* LW;
    double* lw_state;
    int64_t* accepts;
    int64_t* sel;        // nullable, nc x n_keep
    int64_t* final_sel;  // nc
    int32_t* cnt;        // nullable, per proposal (zeroed by caller)
    int32_t* cnt_carry;  // nullable, per chain
    int64_t carry_col;   // >= 0: sel of a state carried in from before the block = carry_col + chain
    double* lw_keep;     // nullable: log weight of kept state k of chain c at lw_keep[c * lw_ld + k]
    int64_t lw_ld;
    uint8_t* acc_step;   // nullable: 1 where step t of chain c accepted, at acc_step[c * acc_ld + t]
    int64_t acc_ld;
    const unsigned int* abort;  // nullable: return at once when *abort & kAbortMask
    // Certified Wang-Ling decisions (LWE non-null, blocked kernels): each decision is
    // taken only when it is the same for every pair of weights within the bounds
    // LWE (proposals) / *emax (chain states carried into the block) of the stored
    // ones; otherwise both weights are recomputed in the reference's order by the
    // wave (wl_exact_wave) and written back with bound 0.
    double* LWE;
    const unsigned long long* emax;
    double* LWx;            // = LW, writable (recomputed weights)
    const double* RT;       // R transposed, d x d (RT[j * d + i] = R[i][j])
    const void* Zst;        // proposal store (coordinate-major, column p, ld ldz, zb-byte elements)
    int zb;
    int64_t ldz;
    const void* zs;         // chain states carried into the block (caller's layout)
    int ob;
    int zs_cm;
    unsigned int* flagw;    // the context's flag words (kFlagWordAcceptResolved, kFlagWordWLMismatch)
    double bscale;          // bounds x bscale (1; a test hook widens them to force recomputations)
    // nullable: the chains' state_init words (lgs.h): >= kInitStep0 = the state is the
    // chain's draw at counter step (word - kInitStep0), so a carried-in state's weight is
    // recomputed with its own uniforms; 1 = initialised, step unknown.  Updated for the
    // chains whose state changes in the block.
    int32_t* state_init;
};
constexpr int32_t kInitStep0 = 2;
__host__ __device__ inline int32_t init_code(uint32_t step) {
    return step <= 0x7fffffffu - (uint32_t)kInitStep0 ? (int32_t)step + kInitStep0 : 1;
}

// Per-series statistics (lgs_diag.hip series_stats_kernel).  Series s starts at
// x + (s / gsize) * gstride + (s % gsize) * sstride, time step t at + t * tstride.
struct SeriesArgs {
    const void* x;
    int xtype;  // 0 fp64, 1 int32, 2 int64
    int64_t n_series, n, gsize, gstride, sstride, tstride;
    int64_t max_lag;  // < 0: mean / batch means only
    double window_c;  // Sokal window constant of the tau_int loop
    int64_t batch;    // > 0: batch means of this size
    double* mean;     // nullable, n_series
    double* c0;       // nullable, n_series: sum (x - mean)^2
    double* acf;      // nullable, n_series x ld_acf (lags 0..min(max_lag, n-1));
                      // null with tau set: lag blocks stop once the window closes
    int64_t ld_acf;
    double* tau;      // nullable, n_series
    double* bmeans;   // nullable, n_series x ld_b
    int64_t ld_b;
};

namespace launch {
// ---- diagnostics (lgs_diag.hip); xtype 0 fp64, 1 int32, 2 int64
hipError_t series_stats(const SeriesArgs& a, hipStream_t st);
// sum y y^T (d x d, both triangles) and sum y (d), y = x - shift (shift nullable),
// ADDED to G / S; x coordinate-major (d x n, ld ldz).  VALU: exact int64 for
// integer x (xtype 1 int32, 2 int64; shift int64), fp64 for xtype 0 (shift fp64).
hipError_t gram(const void* Z, int xtype, int64_t ldz, int d, int64_t n, const void* shift, void* G,
                void* S, hipStream_t st, const unsigned int* gate = nullptr);
// int8-digit path: pack y = x - shift into digit planes Ph / Pl ((d rounded up to
// 128) rows x ldp bytes, ldp = n rounded up to 64; sets kFlagI8Range when some
// |y| > 32639), then the MFMA Gram of the planes (upper block triangle + mirror:
// G must be symmetric on entry).
hipError_t gram_pack(const void* X, int xtype, bool coord_major, int64_t ldx, int d, int64_t n,
                     const long long* shift, int8_t* Ph, int8_t* Pl, int64_t ldp, unsigned int* flags,
                     hipStream_t st);
hipError_t gram_planes(const int8_t* Ph, const int8_t* Pl, int64_t ldp, int d, void* G, void* S,
                       hipStream_t st, const unsigned int* gate = nullptr);
hipError_t jump(const void* x, int xtype, int64_t n, int d, int64_t ld, double* out, hipStream_t st);
hipError_t tvd_minmax(const void* x, int xtype, int64_t n, int d, long long* mn, long long* mx,
                      unsigned int* flags, hipStream_t st);
hipError_t tvd_hist(const void* x, int xtype, int64_t n, int d, const long long* mn,
                    const long long* off, unsigned int* cnt, hipStream_t st);
hipError_t tvd_sum(const unsigned int* c1, const unsigned int* c2, const long long* off, int d,
                   int64_t n1, int64_t n2, double* out, hipStream_t st);
// binned histogram (compute_tvd's bins branch): per-column fp64 range as ordered
// int64 keys (mn / mx must start at +/- the extreme key), converted by
// hist_keys_to_f64; counts of numpy's equal-width bins ADDED to cnt (d x nb)
hipError_t hist_range(const void* x, int xtype, int64_t n, int d, long long* mn, long long* mx,
                      unsigned int* flags, hipStream_t st);
hipError_t hist_keys_to_f64(const long long* mn, const long long* mx, int d, double* lo, double* hi,
                            hipStream_t st);
hipError_t hist_counts(const void* x, int xtype, int64_t n, int d, int64_t nb, const double* edges,
                       const double* fd, unsigned long long* cnt, hipStream_t st);

// zb / ob / ib: coefficient element width in bytes (2, 4 or 8)
hipError_t klein(const KleinArgs& a, const double* R, const double* RP, const double* RC,
                 int panel, int kernel, bool wl, int zb, void* Z, hipStream_t st);
// ka: the launch's Klein arguments (certified Wang-Ling decisions recompute weights)
hipError_t accept(const AcceptArgs& a, const KleinArgs& ka, hipStream_t st);
hipError_t samplez_probe(const double* mu, const double* sig, const double* u, int64_t n,
                         int precision, int linear, int mode, const double* etab, int64_t* z, double* ln,
                         hipStream_t st);
hipError_t log_density(const KleinArgs& a, const double* R, const void* Z, int zb, double* out,
                       hipStream_t st);
// moments of the proposal store + (fsel non-null) the chains' final states into zs
// abort (nullable) below: the kernel returns at once when *abort & kAbortMask
hipError_t moments_final(const void* Z, int zb, int64_t ldz, const int32_t* cnt, int64_t n, int64_t T,
                         const int64_t* fsel, int d, unsigned long long* mom, void* zs, int ob,
                         int zs_cm, int64_t nc, hipStream_t st, const unsigned int* abort,
                         const uint8_t* znz = nullptr, int64_t zlanes = 0, int zshift = 0,
                         const unsigned int* need = nullptr);
hipError_t moments_carry(const void* zs, int zb, int coord_major, int64_t nc, int d,
                         const int32_t* cc, unsigned long long* mom, hipStream_t st,
                         const unsigned int* abort = nullptr, const unsigned int* need = nullptr);
hipError_t gather_z(const void* Z, int zb, int64_t ldz, const int64_t* sel, int64_t nq,
                    int64_t q_per_chain, const void* zs, int ob, int zs_coord_major, int64_t nc,
                    int d, void* out, int out_coord_major, hipStream_t st,
                    const unsigned int* abort = nullptr);
// initial IMHK draws decided on the device: uninit_scan sets *any when some
// init[c] == 0; init_apply (gated by *any, abortable) gives each such chain the
// proposal of column c of Z (ld nc) and its log weight LW[c], and marks it initialised
hipError_t uninit_scan(const int32_t* init, int64_t nc, unsigned int* any, hipStream_t st);
// (flags: the context's flag words; init_apply also checkpoints the resolved count)
hipError_t init_apply(const void* Z, int zb, int32_t* init, int64_t nc, int d, const double* LW, void* zs,
                      int ob, int zs_cm, double* lws, unsigned int* flags, hipStream_t st);
hipError_t transpose_out(const void* Z, int zb, int64_t ldz, int64_t n, int d, void* out, int ob,
                         hipStream_t st);
hipError_t to_coord_major(const void* in, int ib, int64_t n, int d, void* Z, int zb, int64_t ldz,
                          hipStream_t st);
// B z of a history-sourced launch (clive): bz_lean_kernel for the tiles whose live
// chunks meet only diagonal blocks of B, bz_i8_kernel from a device worklist for the
// rest.  offd, bdiag, town: the basis's tables (lgs_bz_host.h); wl: the worklist, one
// count and one word per tile (null: every tile in bz_i8_kernel's direct grid);
// wl_grid: workgroups of the worklist launch; tiles (nullable): device counters, [0]
// tiles bz_lean_kernel computed, [1] tiles bz_i8_kernel did (lgs_bz_tiles).
struct BzLean {
    const unsigned int* offd;
    const int* bdiag;
    const unsigned char* town;
    unsigned int* wl;
    int wl_grid;
    unsigned long long* tiles;
    int pad_lds;  // unused LDS bytes added to each bz_lean_kernel workgroup (caps its workgroups per CU)
};
// V row of sample s: (s / rb) * rstride + roff + s % rb (rb = n, rstride = roff = 0: row s)
hipError_t bz(const void* Z, int zb, int64_t ldz, const int64_t* sel, const double* BT, int d,
              int64_t n, double* V, int64_t ldv, int64_t rb, int64_t rstride, int64_t roff,
              hipStream_t st, const unsigned int* abort = nullptr, const unsigned int* need = nullptr);
hipError_t bz_i8(const void* Z, int zb, int64_t ldz, const int64_t* sel, const int* kchunk,
                 const int* koff, const int8_t* Bd1, const int8_t* Bd0, int dc, int d, int64_t n,
                 double* V, int64_t ldv, int64_t rb, int64_t rstride, int64_t roff,
                 unsigned int* flags, const int16_t* h16, int64_t h16_lanes, int64_t hcols,
                 hipStream_t st, const unsigned int* abort = nullptr, const uint8_t* znz = nullptr,
                 const unsigned int* clive = nullptr, int64_t clive_ld = 0, double* VNP = nullptr,
                 int64_t vn_n = 0, unsigned long long* MP = nullptr, int64_t mp_ld = 0,
                 unsigned int* MPL = nullptr, const BzLean* lean = nullptr);
// moments of the kept states from bz_i8's per-(tile, coordinate) partials MP (packed
// sum over the tile's 64 rows of z^2 * 2^24 + z + 32768; MPL: the tile's live-chunk
// words, (d + 2047) / 2048 per tile), added to mom (2d); returns at once when *flags has
// kFlagI8Range (the gated moments pass replaces it then)
hipError_t bz_moments_reduce(const unsigned long long* MP, const unsigned int* MPL, int64_t ntiles, int64_t mp_ld,
                             int d,
                             unsigned long long* mom, const unsigned int* flags, hipStream_t st,
                             const unsigned int* abort);
// the chains' states after a block from the int16 history of the block's Klein launch:
// zs[c] = proposal fsel[c] (kept as is when fsel[c] < 0); history [d / 16][lanes][16] of z + 128
hipError_t final_h16(const int16_t* h16, int64_t lanes, const int64_t* fsel, int64_t nc, int d, void* zs,
                     int ob, int zs_cm, hipStream_t st, const unsigned int* abort);
// VNP (nullable, 2 ceil(d / 128) x vn_n): per-(half coordinate tile, row) partial sums of
// ||v||^2 of rows q < vn_n (bz_i8), summed per row into VN by vnorm2_reduce (n = vn_n)
hipError_t vnorm2_reduce(const double* VNP, int d, int64_t n, int64_t rb, int64_t rstride, int64_t roff,
                         double* VN, hipStream_t st, const unsigned int* abort = nullptr);
// scalar functionals of kept states: coefficient k of selection q, and
// ||v||^2 of the rows of V (row index (q / rb) * rstride + roff + q % rb in both)
// lag-L sums of nc per-chain series (int64, or fp64 scaled by scale), T new values each
// (row stride ldx), continued through ring (nc x L); sums (L + 2: lags 0..L, then sum x)
// added to; P scratch of (L + 2) nc values
hipError_t lag_update(const void* X, int is_f64, int64_t ldx, int64_t nc, int64_t Tn, int L, double scale,
                      void* ring, void* sums, void* P, hipStream_t st, const unsigned int* abort = nullptr);
hipError_t coord_gather(const void* Z, int zb, int64_t ldz, const int64_t* sel, int64_t nq, int64_t q_per_chain,
                        const void* zs, int ob, int zs_coord_major, int64_t nc, int d, int k, int64_t* out,
                        int64_t rb, int64_t rstride, int64_t roff, hipStream_t st, const unsigned int* abort);
hipError_t vnorm2_rows(const double* V, int d, int64_t n, int64_t rb, int64_t rstride, int64_t roff, double* VN,
                       hipStream_t st, const unsigned int* abort = nullptr, const unsigned int* need = nullptr);
// ---- decoding
// V (row-major n x d) = rows s: sum_c MT[c][r] X[c][s], X coordinate-major fp64 (fp64 MFMA)
hipError_t gemm_f64(const double* X, int64_t ldx, const double* MT, int d, int64_t n, double* V,
                    hipStream_t st);
hipError_t nearest_plane(int d, int64_t n, int panel, const double* RP, const double* RC,
                         const double* rii, const double* CP, int64_t ldc, int zb, void* Z, int64_t ldz,
                         unsigned int* flags, hipStream_t st);
// Klein draws around per-sample centres CP (coordinate-major, CP[i * ldc + p], every lane of
// [0, a.n) readable; zb 4 or 8).  exact: the reference's order; else the blocked certified
// kernel, fp64 MFMA far field (a.n % 64 == 0, a.ldz % 4 == 0, Z 16-byte aligned);
// dmu_scale multiplies the certificate's bound (1; > 1 forces reference-order decisions)
hipError_t klein_targets(const KleinArgs& a, const double* R, const double* RP, const double* RC, int panel,
                         bool exact, const double* CP, int64_t ldc, double dmu_scale, int zb, void* Z,
                         hipStream_t st);
// lgs_klein_decode: K draws per target, lane p = t K + k.  klein_decode is klein_targets
// with the centre of lane p in column p / K of CP (ceil(a.n / K) columns readable) and two
// per-lane outputs: D[p], the kernel's own squared distance ||t - B z||^2 of the draw, and
// E[p] >= |D[p] - D_ref[p]|, a rigorous bound against the reference-order distance (0 with
// exact, where D is that distance).
hipError_t klein_decode(const KleinArgs& a, const double* R, const double* RP, const double* RC, int panel,
                        bool exact, const double* CP, int64_t ldc, double dmu_scale, int zb, void* Z,
                        const DecodeLanes& dl, hipStream_t st);
// lgs_imhk_targets: klein_decode's lanes and centres with the counters of counter_mode 1
// (a.nt = wl.K) and Wang-Ling weights: a.LW[p] the lane's log weight as the kernel formed
// it, a.LWE[p] >= |a.LW[p] - reference-order weight| (0 with exact).
hipError_t klein_imhk_targets(const KleinArgs& a, const double* R, const double* RP, const double* RC, int panel,
                              bool exact, const double* CP, int64_t ldc, double dmu_scale, int zb, void* Z,
                              const WeightLanes& wl, hipStream_t st);
// The certified Metropolis scan over each chain's K draws, a wave per chain (ka: the
// sampling launch's arguments, for the weights recomputed in the reference's order)
hipError_t imhk_targets_accept(const ImhkTargetsArgs& a, const KleinArgs& ka, hipStream_t st);
// Per target t < m: the draw of columns t K .. t K + K - 1 with the smallest
// reference-order distance, ties to the smallest k.  Candidates are the draws whose interval
// [D - E, D + E] reaches below min_k (D_k + E_k); a single candidate wins, several are
// compared at their reference-order distance (RT = R transposed, row-major d x d; Z
// coordinate-major, ld ldz; CP as above).  win[t] = the winner's column, best[t] = its k,
// dist2[t] = its reference-order distance (always recomputed); *resolved counts the targets
// that needed more than one such evaluation; a non-finite distance sets kFlagNonFinite.
// d <= 4032: a workgroup per target, the draw's coefficients staged in LDS and the rows
// shared by up to 16 waves; larger d, or stage_ok = false: a wave per target reading the
// store.
hipError_t decode_select(int d, int64_t m, int64_t K, const double* D, const double* E, const double* RT,
                         const double* CP, int64_t ldc, const void* Z, int zb, int64_t ldz, int64_t* win,
                         int64_t* best, double* dist2, unsigned int* flags, hipStream_t st,
                         bool stage_ok = true);
// Winners' columns of Z into the compact coordinate-major store W (ld ldw >= m; columns
// m .. ldw - 1 zeroed) and, if out != nullptr, into out[t * st_t + i * st_i] (the
// caller's layout), both of width zb.
hipError_t decode_gather(int d, int64_t m, const int64_t* win, const void* Z, int zb, int64_t ldz, void* W,
                         int64_t ldw, void* out, int64_t st_t, int64_t st_i, hipStream_t st);
// ---- exact closest vector (lgs_cvp.hip)
// One launch of the enumeration: every slot of [0, a.nslots) advances its target's search by
// at most a.slice nodes; an idle slot (and one whose target stops) takes the next target
// from a.ctl[0].  zb 4 or 8: the element width of a.W.  d <= kCvpMaxD.
hipError_t cvp_enum(const CvpArgs& a, int zb, hipStream_t st);
// Slots map[0 .. nlive) of src into slots 0 .. nlive - 1 of dst (blocks of S slots each)
hipError_t cvp_compact(const CvpState& src, const CvpState& dst, int64_t S, const int32_t* map, int64_t nlive,
                       int d, hipStream_t st);
// ---- exact closest vector over a batch of bases (lgs_cvpb.hip)
// cvpb_check: a non-finite value among the n doubles of x sets kFlagNonFinite in *flags.
// cvpb_qr: QR(p) of the chunk's m bases with their targets into a.R / a.CP / a.cprime /
// a.qr_status, and every problem's phase (a refused basis: done, status 3).  cvpb_enum: one
// launch over the a.nlive bases of a.live_in, each problem advanced by at most a.slice nodes.
// cvpb_finish: z (zb 4 or 8), v, dist2, nodes and status of the chunk's problems.
hipError_t cvpb_check(const double* x, int64_t n, unsigned int* flags, hipStream_t st);
hipError_t cvpb_qr(const CvpbArgs& a, hipStream_t st);
hipError_t cvpb_enum(const CvpbArgs& a, hipStream_t st);
hipError_t cvpb_finish(const CvpbArgs& a, int zb, hipStream_t st);
// cvpb_qr for a caller without a search (lgs_klein_bases): the same kernel and arithmetic;
// a.CP, a.st and a.pstatus may be null and are then not written.
hipError_t cvpb_qr_only(const CvpbArgs& a, hipStream_t st);
// ---- Klein draws over a batch of bases (lgs_kleinb.hip)
// kleinb_draw: every draw of the chunk into a.ZW / a.DW (a refused basis: zero rows, +inf).
// kleinb_select: per problem the draw with the smallest distance, ties to the smallest index,
// into a.z / a.v / a.best / a.dist2 / a.status.
hipError_t kleinb_draw(const KleinbArgs& a, hipStream_t st);
hipError_t kleinb_select(const KleinbArgs& a, hipStream_t st);
// kleinb_draw_wl: kleinb_draw on the counters (chain, step) of lgs_imhk_bases, the Wang-Ling
// log weight of every draw in a.DW instead of its distance (a refused basis: -inf).
// imhkb_scan: every chain's Metropolis scan over its S1 weights.  imhkb_gather: the final and the kept states out of
// the draws, the final states' lattice points and the problems' status.
hipError_t kleinb_draw_wl(const KleinbArgs& a, hipStream_t st);
hipError_t imhkb_scan(const ImhkbArgs& a, hipStream_t st);
hipError_t imhkb_gather(const ImhkbArgs& a, hipStream_t st);
// ---- exact Gaussian mass (lgs_cvp.hip)
// One launch of the fixed-radius enumeration, as cvp_enum: every slot advances its work item
// by at most a.slice nodes and takes the next waiting item when it stops.  moments: the
// sum_z accumulators (d <= kMassMomentsMaxD).
hipError_t mass_enum(const MassArgs& a, bool moments, hipStream_t st);
// The listing pass over the same items: the same traversal, every point written as a row
// (MassArgs::it_first .. l_rows; it_tgt is required) instead of summed.
hipError_t mass_list(const MassArgs& a, hipStream_t st);
hipError_t mass_compact(const MassState& src, const MassState& dst, int64_t S, const int32_t* map, int64_t nlive,
                        int d, bool moments, hipStream_t st);
// ---- LLL basis reduction (lgs_lll.hip)
// lll_init: the state blocks of the chunk's m bases from a.basis (Gram matrix, U = I, chol(0),
// k = 1); an entry out of range sets kLllFlagRange.  lll_reduce: one launch of the reduction
// over the a.nlive bases of a.live_in.
hipError_t lll_init(const LllArgs& a, hipStream_t st);
hipError_t lll_reduce(const LllArgs& a, hipStream_t st);
// ---- BKZ basis reduction (lgs_bkz.hip): one launch over the a.l.nlive bases of a.l.live_in; the
// state blocks come from lll_init with state_words = bkz_state_words(d), the rest zeroed.
hipError_t bkz_reduce(const BkzArgs& a, hipStream_t st);
// The exact sampler's table (lgs_exact.hip): w and the blocked running sum of every row, in
// three launches -- weights and c_m per block, P_b and M per target, S_m = P_b + c_m -- and
// the draws of one chunk (tb / ob: the element widths of the table's rows and of a.W).
hipError_t exact_scan(const ExactTable& t, const double* shift, double two_s2, hipStream_t st);
hipError_t exact_draw(const ExactDrawArgs& a, int tb, int ob, hipStream_t st);
hipError_t round_coeffs(const double* W, int64_t ldw, int d, int64_t n, int zb, void* Z, int64_t ldz,
                        unsigned int* flags, hipStream_t st);
hipError_t check_range16(const void* zs, int ob, int64_t count, unsigned int* flags, hipStream_t st);
// (a value that does not fit a 16-bit store sets kFlagCarry16 in *flags)
hipError_t carry_cols(const void* zs, int ob, int zs_coord_major, int64_t nc, int d, void* Z, int zb,
                      int64_t ldz, int64_t col0, hipStream_t st, unsigned int* flags = nullptr);
}  // namespace launch
}  // namespace lgs
