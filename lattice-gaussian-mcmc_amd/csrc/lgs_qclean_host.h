// lgs_qclean_host.h -- host side of the q-panel skip's clean state (plain C++, no
// device code: tests/test_qclean_host.py compiles it on its own).
//
// The Klein kernel keeps one byte per (wave, 32-row panel) next to a coefficient
// store: nonzero when that wave's Z rows, int16 history blocks and znz bytes of the
// panel hold the values a skipped panel stores (KleinArgs::qclean).  A launch may read
// those bytes only while the host can prove that the last writer of the store's Z,
// H16 and ZNZ was an int8-digit reference-mode Klein launch with the same geometry.
// QKey is that proof: what the last such launch looked like.  A launch that differs
// in any field runs with the reset flag (every panel dirty, every byte rewritten);
// every other writer of the three buffers drops the key.
#pragma once
#include <cstdint>

namespace lgs {

struct QKey {
    bool valid = false;
    // the allocations, by serial number (an address can come back after a free)
    uint64_t z_id = 0, h16_id = 0, znz_id = 0, state_id = 0;
    // the pointers the launch wrote through
    const void* Z = nullptr;
    const void* H16 = nullptr;
    const void* ZNZ = nullptr;
    // geometry: which bytes each wave owns
    int64_t ldz = 0, h16_lanes = 0, n = 0;
    int h16_shift = 0, d = 0, zb = 0;
    // the lanes' meaning (lgs_imhk: another first chain or chain count is another run)
    int counter_mode = 0;
    uint32_t chain0 = 0;
    uint64_t basis_gen = 0;  // which lgs_set_basis call loaded the basis
    // not compared: a launch gated on this device word (lgs_imhk's initial draws) has
    // been enqueued into the store since; it wrote if and only if the word is nonzero.
    // Only the device knows, so the next launch that claims the key passes the word on
    // (KleinArgs::qclean_gate) and resets itself if it is set.  Valid while the word
    // is: whoever clears the flag words first drops such a key (qkey_flags_cleared).
    const unsigned int* dirty_if = nullptr;

    bool same(const QKey& o) const {
        return z_id == o.z_id && h16_id == o.h16_id && znz_id == o.znz_id && state_id == o.state_id && Z == o.Z &&
               H16 == o.H16 && ZNZ == o.ZNZ && ldz == o.ldz && h16_lanes == o.h16_lanes && n == o.n &&
               h16_shift == o.h16_shift && d == o.d && zb == o.zb && counter_mode == o.counter_mode &&
               chain0 == o.chain0 && basis_gen == o.basis_gen;
    }
};

// A launch described by `launch` is about to write the store whose key is `cur`:
// returns whether it may trust the stored state (false: launch with the reset flag),
// and makes `cur` describe this launch.  *gate: the device word the launch must check
// when trusted (nullptr: none).
inline bool qkey_claim(QKey& cur, const QKey& launch, const unsigned int** gate) {
    const bool trusted = cur.valid && cur.same(launch);
    *gate = trusted ? cur.dirty_if : nullptr;
    cur = launch;
    cur.valid = true;
    cur.dirty_if = nullptr;
    return trusted;
}

// A launch gated on the device word `gate` is enqueued into the store: one pending
// word at most, a second one drops the key.
inline void qkey_gated_write(QKey& cur, const unsigned int* gate) {
    if (cur.dirty_if != nullptr && cur.dirty_if != gate) cur.valid = false;
    cur.dirty_if = gate;
}

// The flag words are being cleared: a key that depends on one is void.
inline void qkey_flags_cleared(QKey& cur) {
    if (cur.dirty_if != nullptr) cur.valid = false;
    cur.dirty_if = nullptr;
}

// Another writer touches the store: its next Klein launch resets.
inline void qkey_drop(QKey& cur) { cur.valid = false; }

}  // namespace lgs
