"""Host side of tests/test_gpu_targets_matrix.py (no GPU).

1. The instantiations klein_targets_zt / klein_targets_any can launch are read out of
   csrc/lgs_kernels.hip -- the store types of klein_targets_any's branches, the lanes argument
   of each public launcher that calls it, the kernels klein_targets_zt names per branch -- and
   the case table of tests/targets_matrix_cases.py must name exactly those: a new
   instantiation without a case, or a case whose kernel is gone, fails here.
2. The device module's docstring accounts for every one of them, and its parametrised ids
   are the ones the table names.
3. Conditions on the inputs of the precision / linear-probabilities matrix, on the oracle
   alone: a kernel that ignored either setting could not pass on the bases added for it.
"""
import fnmatch
import os
import re

import numpy as np

import targets_matrix_cases as C
from conftest import PKG, REPO

SRC = open(os.path.join(PKG, "csrc", "lgs_kernels.hip")).read()
GPU_MODULE = os.path.join(REPO, "tests", "test_gpu_targets_matrix.py")


def _body(signature):
    """Source text of the function whose header matches `signature`, to its closing brace."""
    m = re.search(signature, SRC)
    assert m, signature
    i = SRC.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(SRC[j], 0)
        j += 1
        if depth == 0:
            return SRC[i:j]


def _source_instantiations():
    """Every kernel instantiation the per-target launchers can launch, spelled as
    targets_matrix_cases.instantiation spells them."""
    zt_fn = _body(r"static hipError_t klein_targets_zt\(const KleinArgs& a,[^{]*\{")
    any_fn = _body(r"static hipError_t klein_targets_any\(const KleinArgs& a,[^{]*\{")
    # klein_targets_any: the store types it casts Z to, one call of klein_targets_zt each
    stores = re.findall(r"return klein_targets_zt\([^;]*\((\w+)\*\)Z, st, lo\.\.\.\);", any_fn)
    assert len(stores) == any_fn.count("klein_targets_zt(") and len(set(stores)) == len(stores), stores
    # the public launchers: what each passes for lo...
    lanes = []
    calls = re.findall(r"return klein_targets_any\(a, R, RP, RC, panel, exact, CP, ldc, dmu_scale, zb, Z, st(.*?)\);", SRC)
    for tail in calls:
        arg = tail.strip(", ")
        if not arg:
            lanes.append(None)
        else:
            m = re.search(rf"const (\w+)& {arg}, hipStream_t st\) \{{", SRC)
            assert m, arg
            lanes.append(m.group(1))
    assert len(lanes) == SRC.count("klein_targets_any(") - 1 and len(set(lanes)) == len(lanes), lanes
    # klein_targets_zt: every launch, by branch
    launches = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)<([^>]*)>\)?,", zt_fn)
    assert len(launches) == zt_fn.count("hipLaunchKernelGGL"), launches
    exact_fn = zt_fn[zt_fn.index("if (exact) {"):zt_fn.index("if (a.n % 64 != 0")]
    exact = re.findall(r"(if constexpr \(sizeof\.\.\.\(LO\) == 0\)"
                       r"|else if constexpr \(\(std::is_same<LO, (\w+)>::value \|\| \.\.\.\)\)|else)"
                       r"\s*hipLaunchKernelGGL\((\w+)<ZT>,", exact_fn)
    assert len(exact) == exact_fn.count("hipLaunchKernelGGL") == len(lanes), exact
    named = {None if cond.startswith("if constexpr") else lane or "else": kernel for cond, lane, kernel in exact}
    rest = [ln for ln in lanes if ln not in named]
    assert len(rest) == 1 and "else" in named, (named, lanes)  # the final else takes the one lanes type left
    named[rest[0]] = named.pop("else")
    panels = re.findall(r"klein_targets_kernel<ZT, (\d+), LO\.\.\.>", zt_fn)
    assert len(panels) == len(launches) - len(exact) and len(set(panels)) == len(panels), panels
    assert re.search(r"if \(panel == 16\)\s*hipLaunchKernelGGL\(\(klein_targets_kernel<ZT, 16, LO\.\.\.>\)", zt_fn)
    out = set()
    for zt in stores:
        for lane in lanes:
            out.add(f"{named[lane]}<{zt}>")
            for pb in panels:
                out.add(f"klein_targets_kernel<{zt}, {pb}" + (f", {lane}>" if lane else ">"))
    return out


def test_case_table_names_every_launchable_instantiation():
    source = _source_instantiations()
    table = C.launched()
    assert len(source) == 18
    assert set(table) == source, (sorted(source - set(table)), sorted(set(table) - source))
    assert all(table[k] for k in table)
    # every cell of the cross runs with tabulated and with libm SampleZ, on every basis
    for inst, cases in table.items():
        assert {z for z in C.SAMPLEZ if any(f"-{z}-" in c for c in cases)} == set(C.SAMPLEZ), inst
    assert set(C.PANELS) == {16, 32} and set(C.STORE_TYPES.values()) == {"int32_t", "int64_t"}


def test_device_module_collects_the_cases_the_table_names():
    """The ids the table names exist in the device module (its parametrisation reads the
    same table), and its docstring lists every instantiation next to a pattern that matches
    the table's cases."""
    import test_gpu_targets_matrix as M
    doc = M.__doc__
    ids = set()
    for test in {t for _, _, t in C.ENTRIES.values()}:
        fn = getattr(M, test)
        names = [m.args[0] for m in fn.pytestmark if m.name == "parametrize"]
        assert names == ["name", "panel,samplez,store", "order"], (test, names)
        for name in C.BASES:
            for v in C.VARIANT_IDS:
                for order in C.ORDERS:
                    ids.add(f"{test}[{name}-{v}-{order}]")
    assert open(GPU_MODULE).read().count("@_cross") == len(C.ENTRIES)
    for inst, cases in C.launched().items():
        lines = [ln for ln in doc.splitlines() if ln.strip().startswith(inst + " ")]
        assert len(lines) == 1, inst
        pattern = lines[0].split()[-1]
        matched = [i for i in ids if fnmatch.fnmatchcase(i, pattern.replace("[", "[[]", 1))]
        want = [i for c in cases for i in ids if fnmatch.fnmatchcase(i, c.replace("[", "[[]", 1))]
        assert matched and sorted(matched) == sorted(want), inst


def test_bases_have_the_layout_edges():
    s = C.make_setups()
    assert {n: s[n]["d"] for n in s} == {"q130": 130, "gauss37": 37, "qary40": 40, "gauss17": 17, "int12": 12}
    d = s["q130"]["d"]
    assert (d // 32, d % 32, d // 16, d % 16) == (4, 2, 8, 2)  # ragged bottom below more than one full panel
    assert s["gauss37"]["d"] % 32 == 5 and s["qary40"]["d"] % 32 == 8 and s["gauss17"]["d"] % 16 == 1
    assert not s["gauss37"]["integral"] and not s["gauss17"]["integral"]
    for name, v in s.items():
        assert v["T"].shape == (C.N_TARGETS, v["d"]) and max(n for n, _ in C.N_FIRST) <= C.N_TARGETS
        lanes = [n * K for n, K, _ in C.decode_cases(v["d"])] + [n * (t + 1) for n, t, _ in C.imhk_cases(v["d"])]
        if v["d"] > 40:
            assert max(lanes) <= 300, (name, lanes)
    assert {c[:2] for c in C.decode_cases(130)} == {(1, 1), (5, 3), (4, 64)}
    for dd in (12, 130):
        assert {t for _, t, _ in C.imhk_cases(dd)} == {6, 30}
        assert all(8 <= n <= 64 for n, _, _ in C.imhk_cases(dd))


def test_precision_and_linear_settings_change_the_oracle(oracle):
    """On the basis of every SampleZ kind precision 3 changes oracle rows, and linear-space
    probabilities take the oracle's fallback and change rows at every precision: a kernel that
    ignored either setting cannot pass there."""
    import test_gpu_targets as tg
    n, first = C.PRECISION_N_FIRST[0]
    s = C.make_kinds_setup()

    def rows(s, precision, linear):
        cp = s["T"][:n]  # (the Q frame)
        z, fb = [], 0
        for k in range(0, n, 7):
            o = oracle.klein(s["R"], cp[k], s["sigma"], 1, seed=tg.SEED, first_sample=first + k, precision=precision,
                             use_log_space=not linear)
            z.append(o["z"][0])
            fb += o["fallbacks"]
        return np.array(z), fb

    assert set(C.PRECISION_BASES) >= {"qary40", "q130"} and C.PRECISIONS == (3, 10, 20) and C.LINEAR == (False, True)
    assert s["qframe"] and "kinds" in C.PRECISION_BASES
    base, fb = rows(s, 10, False)
    assert fb == 0
    z3, _ = rows(s, 3, False)
    assert (z3 != base).any(axis=1).sum() >= len(base) // 4
    for precision in C.PRECISIONS:
        zlog, _ = rows(s, precision, False)
        zlin, fb = rows(s, precision, True)
        assert fb > 0 and (zlin != zlog).any(axis=1).sum() >= len(base) // 4, precision
    assert np.abs(base).max() < 2 ** 31
