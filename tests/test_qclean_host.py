"""Host side of the q-panel skip's clean state (csrc/lgs_qclean_host.h), without a device:
the key that lets a Klein launch trust the stored state is compared field by field, a
launch that differs in any field resets and becomes the new key, and a dropped key resets
the next launch whatever it looks like.  The header is plain C++; a small driver compiled
here exercises it.  Which call sites of lgs_capi.hip drop the key (lgs_set_basis, the
other writers of the store, a discarded look-ahead launch) needs a device to run and is
covered by tests/test_gpu_qskip_clean.py; here only a tripwire that each of them is still
there."""
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "lattice-gaussian-mcmc_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include "lgs_qclean_host.h"
using lgs::QKey;
static int bad = 0;
#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); ++bad; } } while (0)
static QKey launch() {
    static int z, h, f;
    QKey k;
    k.z_id = 3; k.h16_id = 4; k.znz_id = 5; k.state_id = 6;
    k.Z = &z; k.H16 = &h; k.ZNZ = &f;
    k.ldz = 4096; k.h16_lanes = 4096; k.n = 4096;
    k.h16_shift = 12; k.d = 100; k.zb = 2;
    k.counter_mode = 1; k.chain0 = 7; k.basis_gen = 2;
    return k;
}
static bool claim(QKey& cur, const QKey& k, const unsigned int** gate = nullptr) {
    const unsigned int* g = nullptr;
    const bool t = lgs::qkey_claim(cur, k, &g);
    if (gate) *gate = g; else CHECK(g == nullptr);
    return t;
}
template <typename F> static void changed(const char* what, F f) {
    QKey cur;
    CHECK(!claim(cur, launch()));  // nothing known yet: reset
    CHECK(claim(cur, launch()));   // the same launch again: trusted
    QKey k = launch();
    f(k);
    if (claim(cur, k)) { std::printf("%s changed, still trusted\n", what); ++bad; }
    CHECK(claim(cur, k));          // the changed launch is the key now
    CHECK(!claim(cur, launch()));  // and the old one resets again
}
int main() {
    static int other;
    changed("Z allocation", [](QKey& k) { k.z_id = 9; });          // reserve: grown, halved, released
    changed("H16 allocation", [](QKey& k) { k.h16_id = 9; });
    changed("ZNZ allocation", [](QKey& k) { k.znz_id = 9; });
    changed("state allocation", [](QKey& k) { k.state_id = 9; });
    changed("Z pointer", [](QKey& k) { k.Z = &other; });
    changed("H16 pointer", [](QKey& k) { k.H16 = &other; });
    changed("ZNZ pointer", [](QKey& k) { k.ZNZ = &other; });
    changed("ldz", [](QKey& k) { k.ldz = 4352; });                 // carried columns
    changed("h16_lanes", [](QKey& k) { k.h16_lanes = 8192; });
    changed("n", [](QKey& k) { k.n = 2048; });                     // another nc or block
    changed("h16_shift", [](QKey& k) { k.h16_shift = 0; });
    changed("d", [](QKey& k) { k.d = 116; });
    changed("store width", [](QKey& k) { k.zb = 4; });             // the int32 / int64 redo
    changed("counter mode", [](QKey& k) { k.counter_mode = 0; });  // lgs_klein after lgs_imhk
    changed("first chain", [](QKey& k) { k.chain0 = 8; });
    changed("basis", [](QKey& k) { k.basis_gen = 3; });            // lgs_set_basis
    QKey cur;
    claim(cur, launch());
    lgs::qkey_drop(cur);  // another writer
    CHECK(!claim(cur, launch()));
    CHECK(claim(cur, launch()));
    // a gated launch (lgs_imhk's initial draws) into the store: the next launch is trusted
    // but has to check the device word; the launch after it has not
    static unsigned int w1, w2;
    const unsigned int* g = nullptr;
    lgs::qkey_gated_write(cur, &w1);
    CHECK(claim(cur, launch(), &g) && g == &w1);
    CHECK(claim(cur, launch(), &g) && g == nullptr);
    // ... unless the flag words were cleared in between, or a second word is pending
    lgs::qkey_gated_write(cur, &w1);
    lgs::qkey_flags_cleared(cur);
    CHECK(!claim(cur, launch(), &g) && g == nullptr);
    lgs::qkey_flags_cleared(cur);  // nothing pending: the key stays
    CHECK(claim(cur, launch()));
    lgs::qkey_gated_write(cur, &w1);
    lgs::qkey_gated_write(cur, &w1);
    CHECK(claim(cur, launch(), &g) && g == &w1);
    lgs::qkey_gated_write(cur, &w1);
    lgs::qkey_gated_write(cur, &w2);
    CHECK(!claim(cur, launch(), &g) && g == nullptr);
    // a gated launch into a store without a key leaves it without one
    QKey none;
    lgs::qkey_gated_write(none, &w1);
    CHECK(!claim(none, launch(), &g) && g == nullptr);
    std::printf("bad %d\n", bad);
    return bad != 0;
}
"""


def test_key_resets_on_every_change(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler (the build itself needs one)"
    src = tmp_path / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "driver"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout


def test_every_field_is_compared():
    """A field added to QKey and forgotten in same() would silently be trusted."""
    hdr = open(os.path.join(CSRC, "lgs_qclean_host.h")).read()
    body = hdr[hdr.index("struct QKey {"):hdr.index("bool same(")]
    fields = []
    for decl in re.findall(r"^\s+(?:const\s+)?[\w:]+\*?\s+([^;()]+);", body, re.M):
        fields += [f.split("=")[0].strip().lstrip("*") for f in decl.split(",")]
    fields = [f for f in fields if f != "valid" and "dirty_if" not in f]  # (dirty_if: a condition on the key)
    same = hdr[hdr.index("bool same("):hdr.index("// A launch described")]
    assert len(fields) == 16, fields
    for f in fields:
        assert re.search(rf"\b{f} == o\.{f}\b", same), f


def test_writers_of_the_store_drop_the_key():
    """A tripwire only, on the source text of lgs_capi.hip: the drops that exist today are
    still where they were (it breaks on a rename, and says nothing about a writer of c->Z
    added later).  What the drops are for is checked on the GPU:
    tests/test_gpu_qskip_clean.py::test_imhk_state_invalidated."""
    src = open(os.path.join(CSRC, "lgs_capi.hip")).read()

    def fn(name):
        s = src[src.index(name):]
        return s[:s.index("\n}\n")]

    rk = fn("int run_klein(lgs_ctx* c")
    assert "lgs::qkey_claim(c->qkey, k, &a.qclean_gate)" in rk and "lgs::qkey_drop(c->qkey)" in rk
    assert "!a.gate" in rk and "lgs::qkey_gated_write(c->qkey, a.gate)" in rk
    for name in ("int finish(lgs_ctx* c", "int finish_or_redo(lgs_ctx* c", "int reset_flags(lgs_ctx* c",
                 "int spec_discard(lgs_ctx* c"):
        assert "qclean_flags_cleared(c)" in fn(name), name
    assert "qkey_drop(c->bset[c->spec.j].qkey)" in fn("int spec_discard(lgs_ctx* c")
    sb = fn("int lgs_set_basis(lgs_ctx* c")
    assert "c->basis_gen += 1" in sb and "qkey_drop(s.qkey)" in sb
    for name in ("int lgs_lattice_points(", "int lgs_log_density("):
        assert "qkey_drop(c->qkey)" in fn(name), name
    # the per-target entry points that write c->Z take it through the shared frame, which drops the key
    take = src[src.index("    void* take_store() {"):]
    assert "qkey_drop(c->qkey)" in take[:take.index("\n    }\n")]
    for name in ("int run_decode(", "int lgs_klein_targets(", "int lgs_klein_decode(", "int lgs_imhk_targets("):
        assert "t.take_store()" in fn(name) and "c->Z.p" not in fn(name), name
    assert "std::swap(c->qkey, s.qkey)" in src and "swap_buf(c->QCL, s.QCL)" in src
