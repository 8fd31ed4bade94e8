// lgs_bz_i8_body.inc -- the body of bz_i8_kernel: one (64 kBzTA samples x kBzBN kBzTxPer
// coordinates) tile of the int8-digit B z.  Included by bz_i8_kernel (tile from blockIdx) and
// by bz_i8_wl_kernel (tiles from a device worklist), which define LGS_BZ_TILE_INDEX: the
// statements that declare the sample tile `ty` (int64_t) and the coordinate-tile group
// `txg` (int).  One text for both, and not a function: the kernel sits at its register
// budget (kBzOcc), and a call frame around the same statements made it spill.
    constexpr int TA = kBzTA;  // 32-sample MFMA tiles per wave
    constexpr int BM = 64 * TA, BN = kBzBN, KC = 64, P = 80;  // P: LDS row pitch (bytes), conflict-free
    constexpr int TN = BN / 64;  // 32-coordinate MFMA tiles per wave (waves 2 x 2)
    constexpr int KPT = KC * BM / 256;  // coefficients per thread per chunk
    __shared__ __attribute__((aligned(16))) int8_t Zs1[BM * P], Zs0[BM * P], Bs1[BN * P], Bs0[BN * P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs, so
    // workgroup b runs on XCD b % 8; the tx_count coordinate tiles of one sample
    // tile are given to consecutive workgroups of the same XCD, which then reads
    // that sample tile's coefficients from HBM once and from its own L2 after.
    // Each workgroup computes kBzTxPer consecutive coordinate tiles of its
    // sample tile, so the output stores of one tile drain while the MFMAs of the
    // next one run.
    LGS_BZ_TILE_INDEX
    if (ty >= ty_count) return;
    const int64_t s0 = ty * BM;
    const int ntx = (d + BN - 1) / BN;
    ZT zmax = 0, zmin = 0;  // range of the coefficients read (exactness check)
    for (int tx = txg * kBzTxPer; tx < ntx && tx < (txg + 1) * kBzTxPer; ++tx) {
    const int r0 = tx * BN;
    v16i_t p1[TA][TN], p2[TA][TN], p3[TA][TN];
#pragma unroll
    for (int ta = 0; ta < TA; ++ta)
#pragma unroll
        for (int t = 0; t < TN; ++t) {
            p1[ta][t] = (v16i_t){};
            p2[ta][t] = (v16i_t){};
            p3[ta][t] = (v16i_t){};
        }
    const int zm = tid & (BM - 1), zq = tid / BM;
    const int64_t zs_ = s0 + zm;
    const int64_t zcol = zs_ < n ? (sel ? sel[zs_] : zs_) : 0;  // this thread's sample column
    // only the K chunks where this row tile of B has a non-zero digit (exact skip)
    // (the block-sparsity lists are per 128-row tile of B)
    const int ci0 = koff[tx * BN / 128];
    const int ci1 = koff[tx * BN / 128 + 1];
    // Chunks where every sample of the tile has z = 0 on all 64 coordinates contribute
    // exactly nothing: skipped.  The Klein launch that wrote the history flags each
    // (16-coordinate block, sample) holding a nonzero (znz); thread (zm, zq) checks
    // block zq of each chunk for its sample, the tile ORs them in LDS.  Samples read
    // from the coefficient store (not that launch's) count as nonzero.  (NTRU / q-ary
    // bases: the q-coordinates' z are 0, which leaves ~1 of 6 chunks per tile.)
    // (round 4) the Klein launch also leaves, per wave, one bit per 64-coordinate chunk
    // (clive): the tile's live chunks are the OR of its samples' waves' words -- one
    // load per 32 chunks and sample instead of one flag load and LDS atomic per chunk
    const bool use_clive = KPT == 16 && h16 != nullptr && clive != nullptr;
    const bool use_znz = !use_clive && KPT == 16 && h16 != nullptr && znz != nullptr;
    __shared__ unsigned int livew[kOzMaxD / 64 / 32];
    // (round 5) every wave ORs the words itself: the 4 waves hold the same 64 samples
    // (zm = lane), so no LDS round trip and barrier precede the first chunk's loads;
    // the word stays in a scalar register up to d = 2048, else in the wave's LDS row
    __shared__ unsigned int livew4[4][kOzMaxD / 64 / 32];
    const int ngw = (d + 2047) / 2048;
    unsigned int live1 = 0u;
    if (use_clive) {
        {
            const int ng = ngw;
            // the word of the identity selection (row q = proposal q: every kept state a
            // fresh proposal, e.g. acceptance 1) is loaded beside the selection itself
            // instead of after it; a lane whose selection differs reloads
            const int64_t zg = zs_ < n ? zs_ : 0;
            const unsigned int wg0 = zg < hcols ? clive[zg >> 6] : 0xffffffffu;
            const bool same = (zcol >> 6) == (zg >> 6) && (zcol < hcols) == (zg < hcols);
            for (int g = 0; g < ng; ++g) {
                unsigned int w = 0u;
                const unsigned int wg =
                    g == 0 ? wg0 : (zg < hcols ? clive[(size_t)g * clive_ld + (zg >> 6)] : 0xffffffffu);
                if (zs_ < n)
                    w = same ? wg : (zcol < hcols ? clive[(size_t)g * clive_ld + (zcol >> 6)] : 0xffffffffu);
                // OR over the wave's lanes; all equal (the tile's samples from one Klein
                // wave) needs no shuffles
                const unsigned int w0 = __builtin_amdgcn_readfirstlane(w);
                if (__builtin_amdgcn_ballot_w64(w != w0) != 0ull) {
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) w |= __shfl_xor(w, o);
                } else {
                    w = w0;
                }
                if (ng == 1)
                    live1 = __builtin_amdgcn_readfirstlane(w);
                else if (lane == 0)
                    livew4[wave][g] = w;
            }
            if (ng > 1) {  // the wave's own LDS row: in order within the wave
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
    // (MP) the tile's live-chunk words for the moments' reduction: a chunk the tile
    // skips leaves its partials unwritten
    if (MP != nullptr && use_clive && tx == 0 && tid < ngw) MPL[(size_t)ty * ngw + tid] = ngw == 1 ? live1 : livew4[0][tid];
    if (use_znz) {
        const bool hp = zs_ < n && zcol < hcols;
        for (int w = tid; w < (ci1 - ci0 + 31) / 32; w += 256) livew[w] = 0u;
        __syncthreads();
        for (int ci = ci0; ci < ci1; ++ci) {
            const int c0 = (kchunk[ci] & 0xffff) * KC;
            const bool nz = zs_ < n && (!hp || znz[(size_t)((c0 + zq * 16) >> 4) * h16_lanes + zcol] != 0);
            if (nz) atomicOr(&livew[(ci - ci0) >> 5], 1u << ((ci - ci0) & 31));
        }
        __syncthreads();
    }
    for (int ci = ci0; ci < ci1; ++ci) {
        // (bit 16 of a chunk entry: this row tile owns the chunk's moments, MP)
        const int kraw = kchunk[ci];
        const int cix = kraw & 0xffff;
        const bool mown = MP != nullptr && (kraw >> 16) != 0 && KPT == 16 && (BN == 128 || (tx & 1) == 0);
        if ((use_clive && !(((ngw == 1 ? live1 : livew4[wave][cix >> 5]) >> (cix & 31)) & 1u)) ||
            (use_znz && !((livew[(ci - ci0) >> 5] >> ((ci - ci0) & 31)) & 1u))) {  // (uniform)
            continue;  // (an all-zero chunk's moment partials stay 0: MP is cleared per launch)
        }
        const int c0 = cix * KC;
        if (KPT == 16 && h16 != nullptr && zs_ < n && zcol < hcols) {
            // column written by the Klein launch whose int16 history (z + 128,
            // [coordinate / 16][lane][16]) holds this sample's 16 coefficients in 32
            // contiguous bytes: the digit planes are byte permutes of them (exact:
            // that launch checked |z| against the history's range)
            const v4u_t* hp = (const v4u_t*)(h16 + ((size_t)((c0 + zq * 16) >> 4) * h16_lanes + zcol) * 16);
            const v4u_t y0 = hp[0], y1 = hp[1];
            v4i_t w0, w1;
            w1[0] = (int)__builtin_amdgcn_perm(y0[1], y0[0], 0x07050301u);
            w1[1] = (int)__builtin_amdgcn_perm(y0[3], y0[2], 0x07050301u);
            w1[2] = (int)__builtin_amdgcn_perm(y1[1], y1[0], 0x07050301u);
            w1[3] = (int)__builtin_amdgcn_perm(y1[3], y1[2], 0x07050301u);
            w0[0] = (int)(__builtin_amdgcn_perm(y0[1], y0[0], 0x06040200u) ^ 0x80808080u);
            w0[1] = (int)(__builtin_amdgcn_perm(y0[3], y0[2], 0x06040200u) ^ 0x80808080u);
            w0[2] = (int)(__builtin_amdgcn_perm(y1[1], y1[0], 0x06040200u) ^ 0x80808080u);
            w0[3] = (int)(__builtin_amdgcn_perm(y1[3], y1[2], 0x06040200u) ^ 0x80808080u);
            *(v4i_t*)&Zs0[zm * P + zq * 16] = w0;
            *(v4i_t*)&Zs1[zm * P + zq * 16] = w1;
        } else {  // z chunk -> balanced base-256 digits, [sample][k] byte planes
            const bool sok = zs_ < n;
            const ZT* zp = Z + (size_t)(c0 + zq * KPT) * ldz + zcol;
#pragma unroll
            for (int h = 0; h < KPT / 16; ++h) {
            v4i_t w0, w1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // z = 256 hi + lo with lo in [-128, 127]: lo's byte is z's low
                // byte and hi = (z + 128) >> 8, whose byte is byte 1 of z + 128;
                // v_perm_b32 gathers four such bytes into one dword
                unsigned int zz[4], hh[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + zq * KPT + h * 16 + q * 4 + j;
                    const ZT zr = (sok && c < d) ? zp[(size_t)(h * 16 + q * 4 + j) * ldz] : (ZT)0;
                    zmax = max(zmax, zr);
                    zmin = min(zmin, zr);
                    zz[j] = (unsigned int)(int)zr;
                    hh[j] = zz[j] + 128u;
                }
                w0[q] = (int)(__builtin_amdgcn_perm(zz[1], zz[0], 0x0c0c0400u) |
                              __builtin_amdgcn_perm(zz[3], zz[2], 0x04000c0cu));
                w1[q] = (int)(__builtin_amdgcn_perm(hh[1], hh[0], 0x0c0c0501u) |
                              __builtin_amdgcn_perm(hh[3], hh[2], 0x05010c0cu));
            }
            *(v4i_t*)&Zs0[zm * P + zq * KPT + h * 16] = w0;
            *(v4i_t*)&Zs1[zm * P + zq * KPT + h * 16] = w1;
            }
        }
#pragma unroll
        for (int e = 0; e < BN / 64; ++e) {  // B digit planes [coord][k], 16 B per thread per plane
            const int idx = tid + 256 * e;
            const int row = idx >> 2, part = idx & 3;
            const size_t g = (size_t)(r0 + row) * dc + c0 + part * 16;
            *(v4i_t*)&Bs1[row * P + part * 16] = *(const v4i_t*)&Bd1[g];
            *(v4i_t*)&Bs0[row * P + part * 16] = *(const v4i_t*)&Bd0[g];
        }
        __syncthreads();
        auto moment_partials = [&]() __attribute__((always_inline)) {
            // (round 5) the kept states' moments ride on this tile's digit planes while the
            // MFMAs run (round 6: called after the chunk's MFMAs are issued, so the VALU work
            // runs under the matrix pipe -- with the 16-byte stores below, B z 7.19 -> 6.98 ms
            // per 2^22 lattice points, profiles/r06q_bz_ab.log):
            // wave w sums coordinates 16w..16w+15 of the chunk over the tile's 64
            // rows, lane (4 coordinates: lane >> 4) x (4 rows: lane & 15), packed per row as
            // z^2 * 2^24 + (z + 32768) (64 rows: the low field < 2^22, the total < 2^63;
            // rows past n hold z = 0 and add the bias only), then over the 16 lanes of a
            // DPP row (row_ror 8, 4, 2, 1: VALU moves, no LDS round trip)
            const int kk = 16 * wave + 4 * (lane >> 4);
            unsigned long long ps[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = 4 * (lane & 15) + i;
                const unsigned int lo4 = *(const unsigned int*)&Zs0[row * P + kk];
                const unsigned int hi4 = *(const unsigned int*)&Zs1[row * P + kk];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int z = 256 * (int)(signed char)(hi4 >> (8 * j)) + (int)(signed char)(lo4 >> (8 * j));
                    ps[j] += ((unsigned long long)(unsigned int)(z * z) << 24) + (unsigned int)(z + 32768);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ps[j] += dpp_row_ror_u64<0x128>(ps[j]);  // row_ror:8
                ps[j] += dpp_row_ror_u64<0x124>(ps[j]);  // row_ror:4
                ps[j] += dpp_row_ror_u64<0x122>(ps[j]);  // row_ror:2
                ps[j] += dpp_row_ror_u64<0x121>(ps[j]);  // row_ror:1
            }
            if ((lane & 15) == 0) {
                unsigned long long* mp = MP + (size_t)ty * mp_ld + c0 + kk;
#pragma unroll
                for (int j = 0; j < 4; ++j) mp[j] = ps[j];
            }
        };
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int kb = ks * 32 + 16 * (lane >> 5);
            v4i_t a1[TA], a0[TA];
#pragma unroll
            for (int ta = 0; ta < TA; ++ta) {
                const int arow = (wm * TA + ta) * 32 + (lane & 31);
                a1[ta] = *(const v4i_t*)&Zs1[arow * P + kb];
                a0[ta] = *(const v4i_t*)&Zs0[arow * P + kb];
            }
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int col = wn * (BN / 2) + tn * 32 + (lane & 31);
                const v4i_t b1 = *(const v4i_t*)&Bs1[col * P + kb];
                const v4i_t b0 = *(const v4i_t*)&Bs0[col * P + kb];
#pragma unroll
                for (int ta = 0; ta < TA; ++ta) {
                    p1[ta][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1[ta], b1, p1[ta][tn], 0, 0, 0);
                    p2[ta][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1[ta], b0, p2[ta][tn], 0, 0, 0);
                    p2[ta][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0[ta], b1, p2[ta][tn], 0, 0, 0);
                    p3[ta][tn] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0[ta], b0, p3[ta][tn], 0, 0, 0);
                }
            }
        }
        if (mown) moment_partials();
        __syncthreads();
    }
    // output rows: sample q -> (q / rb) * rstride + roff + q % rb.  The wave's 32
    // rows start at qb (wave-uniform); with rb >= 32 they cross at most one block
    // boundary, so each row's address is a uniform base + row * ldv + (one
    // uniform jump past the boundary) -- no per-row division or 64-bit multiply.
    // v = 65536 p1 + 256 p2 + p3 is formed in fp64: every partial sum is an
    // integer below 2^53, so it is exact (and equal to the int64 combination).
    const int lrow = 4 * (lane >> 5);
#pragma unroll
    for (int ta = 0; ta < TA; ++ta) {
    const int64_t qb = s0 + (wm * TA + ta) * 32;
    if (VNP && qb < vn_n) {
        // ||v||^2 of the tile's rows (a scalar functional of the kept states, SURVEY
        // 8e): one partial sum per (row, 64-coordinate half tile), stored to its own
        // slot VNP[(2 tx + wn) vn_n + q] and summed per row by vnorm2_reduce_kernel (atomics
        // on the 64 rows' few cache lines from 16 workgroups serialised: 0.5 ms per 2^20).
        // Only the rows q < vn_n (the leading chains a lag series follows): computed for
        // every row this epilogue cost 0.94 ms per 2^20 (bz 1.70 -> 2.65 ms).
        // Lane & 31 is the coordinate: the 16 rows' partial sums are reduced over the 32
        // lanes by halving (16 shuffles instead of 80).  Integral v: exact in any order.
        double vs[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            vs[reg] = 0.0;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                if (r0 + wn * (BN / 2) + tn * 32 + (lane & 31) < d) {
                    const double v = fma((double)p1[ta][tn][reg], 65536.0, (double)p2[ta][tn][reg] * 256.0) +
                                     (double)p3[ta][tn][reg];
                    vs[reg] = fma(v, v, vs[reg]);
                }
        }
        int ridx = 0;
#pragma unroll
        for (int half = 8; half >= 1; half >>= 1) {  // lane bit 16 -> 8 values, bit 8 -> 4, ...
            const int bit = half * 2;
            const bool up = (lane & bit) != 0;
#pragma unroll
            for (int j = 0; j < half; ++j) {
                const double send = up ? vs[j] : vs[j + half];
                const double keep = up ? vs[j + half] : vs[j];
                vs[j] = keep + __shfl_xor(send, bit);
            }
            ridx += up ? half : 0;
        }
        const double tot = vs[0] + __shfl_xor(vs[0], 1);
        const int row = (ridx & 3) + 8 * (ridx >> 2) + lrow;
        const int64_t q = qb + row;
        if (!(lane & 1) && q < vn_n) VNP[(size_t)(2 * tx + wn) * vn_n + q] = tot;
    }
    const int64_t cb = qb / rb;
    const int64_t kb0 = qb - cb * rb;
    const int nrow = (int)min<int64_t>(n - qb, 32);  // valid rows of this tile
    // (round 6, with the moments after the MFMAs: B z 7.19 -> 6.98 ms per 2^22 lattice
    // points, profiles/r06q_bz_ab.log) 16-byte stores: lanes 2c and 2c + 1 swap one value per pair of rows
    // (DPP quad_perm [1, 0, 3, 2]), so the even lane holds row r, columns 2c and 2c + 1
    // and the odd lane row r + 1, the same columns (even d and ldv, V 16-byte aligned: every
    // pair then starts on a 16-byte boundary; otherwise the 8-byte stores below)
    if (rb >= 32 && (d & 1) == 0 && (ldv & 1) == 0 && ((uintptr_t)V & 15) == 0) {
        typedef double v2d_t __attribute__((ext_vector_type(2)));
        const int wrap_row = (int)min<int64_t>(rb - kb0, 32);
        const bool odd = (lane & 1) != 0;
        const int c = r0 + wn * (BN / 2) + ((lane & 31) & ~1);
        double* const vbase = V + (size_t)(cb * rstride + roff + kb0) * ldv + c;
        const int64_t jump = (rstride - rb) * ldv;
#pragma unroll
        for (int reg = 0; reg < 16; reg += 2) {
            const int row = (reg & 3) + 8 * (reg >> 2) + lrow + (odd ? 1 : 0);
            double* vrow = vbase + (size_t)row * ldv + (row >= wrap_row ? jump : 0);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const double va = fma((double)p1[ta][tn][reg], 65536.0, (double)p2[ta][tn][reg] * 256.0) +
                                  (double)p3[ta][tn][reg];
                const double vb = fma((double)p1[ta][tn][reg + 1], 65536.0, (double)p2[ta][tn][reg + 1] * 256.0) +
                                  (double)p3[ta][tn][reg + 1];
                const double send = odd ? va : vb;
                const unsigned long long sb = __double_as_longlong(send);
                const unsigned int rlo = (unsigned int)__builtin_amdgcn_mov_dpp((int)(unsigned int)sb, 0xb1, 0xf, 0xf, false);
                const unsigned int rhi = (unsigned int)__builtin_amdgcn_mov_dpp((int)(unsigned int)(sb >> 32), 0xb1, 0xf, 0xf, false);
                const double recv = __longlong_as_double((long long)(((unsigned long long)rhi << 32) | rlo));
                v2d_t o;
                o[0] = odd ? recv : va;
                o[1] = odd ? vb : recv;
                if (row < nrow && c + tn * 32 < d) __builtin_nontemporal_store(o, (v2d_t*)(vrow + tn * 32));
            }
        }
    } else
    if (rb >= 32) {
        const int wrap_row = (int)min<int64_t>(rb - kb0, 32);  // first row past the boundary
        double* const vbase = V + (size_t)(cb * rstride + roff + kb0) * ldv + r0 + wn * (BN / 2) + (lane & 31);
        const int64_t jump = (rstride - rb) * ldv;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + lrow;
            if (row >= nrow) continue;
            double* vrow = vbase + (size_t)row * ldv + (row >= wrap_row ? jump : 0);
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                if (r0 + wn * (BN / 2) + tn * 32 + (lane & 31) < d) {
                    const double v = fma((double)p1[ta][tn][reg], 65536.0, (double)p2[ta][tn][reg] * 256.0) +
                                     (double)p3[ta][tn][reg];
                    __builtin_nontemporal_store(v, vrow + tn * 32);  // streamed out, not re-read
                }
            }
        }
    } else {
        const unsigned int ukb0 = (unsigned int)kb0, urb = (unsigned int)rb;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = (reg & 3) + 8 * (reg >> 2) + lrow;
            if (row >= nrow) continue;
            const unsigned int kk = ukb0 + (unsigned int)row;
            const unsigned int wrap = kk / urb;
            const int64_t orow = (cb + wrap) * rstride + roff + (kk - wrap * urb);
            double* vrow = V + (size_t)orow * ldv;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) {
                const int r = r0 + wn * (BN / 2) + tn * 32 + (lane & 31);
                if (r < d) {
                    const double v = fma((double)p1[ta][tn][reg], 65536.0, (double)p2[ta][tn][reg] * 256.0) +
                                     (double)p3[ta][tn][reg];
                    __builtin_nontemporal_store(v, vrow + r);
                }
            }
        }
    }
    }
    }
    if (zmax > (ZT)32639 || zmin < (ZT)-32639) atomicOr(flags, kFlagI8Range);
