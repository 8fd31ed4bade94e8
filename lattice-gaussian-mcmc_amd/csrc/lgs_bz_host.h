// lgs_bz_host.h -- host side of B z's diagonal-only tiles (plain C++, no device code:
// tests/test_bz_host.py compiles it on its own).
//
// bz_lean_kernel computes a (64 samples x 128 coordinates) tile of v = B z without the
// digit GEMM when every live 64-coordinate chunk of the tile's samples meets a block of
// B with nothing off its diagonal: v_j = B_jj z_j then.  A block is (128-row tile tx of
// B, 64-column chunk ch); its rows and columns are both global coordinates, so its
// diagonal is the entries (r, c) with r == c, and only the blocks ch = 2 tx, 2 tx + 1 on
// B's main diagonal have one (q-ary / NTRU bases [[qI, 0], [A, I]]; nothing more general
// is looked for).  lgs_set_basis builds these tables once per basis.
#pragma once
#include <cstdint>
#include <vector>

namespace lgs {

struct BzTileTables {
    int words = 0;                    // words per tile in offd
    std::vector<unsigned int> offd;   // [tile][words]: bit ch & 31 of word ch >> 5 set when block
                                      // (tile, ch) has a nonzero entry off its diagonal
    std::vector<int> bdiag;           // B_jj, zero-padded to whole tiles
    std::vector<unsigned char> town;  // [tile]: bit e set when the tile is the first (lowest) one
                                      // whose block on chunk 2 tile + e is nonzero: it owns the
                                      // chunk's moment partials (bit 16 of lgs_set_basis's kchunk)
    bool any_lean = false;            // some tile's own blocks are diagonal: only then is
                                      // bz_lean_kernel worth launching
};

// B: row-major d x d, integral entries that fit an int.
inline BzTileTables bz_tile_tables(const double* B, int64_t d, int words) {
    BzTileTables t;
    const int64_t ntile = (d + 127) / 128, nchunk = (d + 63) / 64;
    t.words = words;
    t.offd.assign((size_t)ntile * words, 0u);
    t.bdiag.assign((size_t)ntile * 128, 0);
    t.town.assign((size_t)ntile, 0);
    std::vector<char> listed((size_t)nchunk, 0);
    for (int64_t j = 0; j < d; ++j) t.bdiag[(size_t)j] = (int)B[j * d + j];
    for (int64_t tx = 0; tx < ntile; ++tx) {
        for (int64_t ch = 0; ch < nchunk; ++ch) {
            bool nz = false, off = false;
            for (int64_t r = tx * 128; r < tx * 128 + 128 && r < d; ++r)
                for (int64_t c = ch * 64; c < ch * 64 + 64 && c < d; ++c)
                    if (B[r * d + c] != 0.0) {
                        nz = true;
                        off = off || r != c;
                    }
            if (off) t.offd[(size_t)tx * words + (ch >> 5)] |= 1u << (ch & 31);
            if (nz && !listed[(size_t)ch]) {
                listed[(size_t)ch] = 1;
                if (ch >> 1 == tx) t.town[(size_t)tx] |= (unsigned char)(1u << (ch & 1));
            }
        }
        bool own_diag = true;
        for (int64_t ch = 2 * tx; ch < 2 * tx + 2 && ch < nchunk; ++ch)
            own_diag = own_diag && !((t.offd[(size_t)tx * words + (ch >> 5)] >> (ch & 31)) & 1u);
        t.any_lean = t.any_lean || own_diag;
    }
    return t;
}

}  // namespace lgs
