"""CPU-side checks of the call-order probe table (tests/call_order_cases.py): it covers every
compute entry point include/lgs.h declares, and the premises its inputs were chosen for hold
on the CPU transcriptions -- every enumeration ends with status 0 well inside its budget, every
tree has more than one node, every ball holds a point, every LLL input needs a swap."""
import numpy as np

import call_order_cases as C
from test_capi_host import declared_symbols


def test_every_declared_symbol_has_a_row_or_a_reason():
    """An entry point added to lgs.h without a row (or a reasoned exclusion) fails here; so does
    a row removed from the table."""
    declared = set(declared_symbols())
    covered = C.covered_symbols()
    assert not covered & set(C.EXCLUDED), sorted(covered & set(C.EXCLUDED))
    missing = declared - covered - set(C.EXCLUDED)
    assert not missing, f"declared in lgs.h, no probe row and no exclusion: {sorted(missing)}"
    stale = (covered | set(C.EXCLUDED)) - declared
    assert not stale, f"rows or exclusions for symbols lgs.h no longer declares: {sorted(stale)}"
    assert all(C.EXCLUDED.values())
    # the exclusions are the set-up, tear-down and getter calls and nothing else
    assert set(C.EXCLUDED) == {"lgs_version", "lgs_last_error", "lgs_create", "lgs_create_ex", "lgs_destroy",
                               "lgs_device_info", "lgs_timing_enable", "lgs_timing_get", "lgs_counter",
                               "lgs_qskip_elided", "lgs_bz_tiles", "lgs_set_basis", "lgs_set_decoder",
                               "lgs_set_stream"}


def test_rows_are_well_formed():
    names = [r.name for r in C.ROWS]
    assert len(set(names)) == len(names)
    # every row by name: several are variants of one symbol (ragged n and whole blocks, reference
    # and Wang-Ling weights, row-major and coordinate-major), which the symbol gate cannot miss
    assert set(names) == {
        "klein_ragged", "klein_blocks", "klein_targets", "klein_decode", "imhk_ref", "imhk_wl", "imhk_trace",
        "imhk_ex", "imhk_targets", "nearest_plane", "round_decode", "lattice_points_rows", "lattice_points_coords",
        "log_density", "sample_z", "closest_vector", "gaussian_mass", "ball_points", "exact_table+exact_sample",
        "lll_reduce", "bkz_reduce", "closest_vector_bases", "klein_bases", "imhk_bases", "series_stats", "gram",
        "jump_distance", "marginal_tvd", "column_range", "histogram"}
    for r in C.ROWS:
        assert r.kinds and set(r.kinds) <= {False, True}, r.name
    # host-only / device-only rows are the ones the header leaves no choice for
    assert {r.name for r in C.ROWS if r.kinds != C.KINDS} == {"sample_z", "imhk_ex"}
    # the enumeration family is the part of the table bound to d <= 64
    assert {r.name for r in C.ROWS if r.max_d} == {"closest_vector", "gaussian_mass", "ball_points",
                                                   "exact_table+exact_sample"}
    assert set(C.NO_BASIS) >= {"lll_reduce", "bkz_reduce", "closest_vector_bases", "klein_bases", "imhk_bases"}
    s, l = C.SIZES["small"], C.SIZES["large"]
    assert (s["nt"], s["ns"], s["nb"]) == (3, 64, 2) and (l["nt"], l["ns"], l["nb"]) == (130, 512, 9)
    assert l["ns"] % 256 == 0 and (l["ns"] - 3) % 64 and (s["ns"] - 3) % 64


def test_subject_enumerations_end_inside_their_budgets():
    """int12 on the CPU transcriptions, every one of the 130 targets: the closest-vector search
    and the fixed-radius traversal end with status 0 in at most half of MAX_NODES nodes (so the
    ulps between the host's c' and the library's cannot reach the budget), visit more than one
    node, every ball holds a point and some hold many, and all the balls fit into half of
    MAX_POINTS rows."""
    import ball_oracle
    import cvp_oracle
    import mass_oracle
    s = C.subject()
    assert s["d"] == 12 and s["sigma"] == 45.0 and s["integral"]
    n = C.SIZES["large"]["nt"]
    total = 0
    for k in range(n):
        cp = s["T"][k] @ s["Q"]
        z, D, nodes, st = cvp_oracle.se(s["R"], cp, max_nodes=C.MAX_NODES)
        assert st == 0 and 1 < nodes <= C.MAX_NODES // 2 and z.any()
        assert D == s["shift"][k] and s["radius2"][k] > D
        m = mass_oracle.enum(s["R"], cp, C.MASS_SIGMA, s["radius2"][k], s["shift"][k], max_nodes=C.MAX_NODES)
        assert m["status"] == 0 and 1 < m["nodes"] <= C.MAX_NODES // 2 and m["points"] >= 1 and m["mass"] >= 1.0
        rows, _, bn, bs = ball_oracle.points(s["R"], cp, s["radius2"][k], C.MAX_NODES)
        assert bs == 0 and bn == m["nodes"] and len(rows) == m["points"]
        total += m["points"]
    assert n < total <= C.MAX_POINTS // 2
    # the small size's three balls hold more rows than targets too (its draws can differ)
    assert sum(len(ball_oracle.points(s["R"], s["T"][k] @ s["Q"], s["radius2"][k])[0]) for k in range(3)) > 3


def test_batched_bases_premises():
    """The nine d = 8 bases: raw, each needs LLL swaps (and the first is lll_oracle's qary8);
    reduced, every one of the 9 x 64 closest-vector problems ends with status 0 in more than one
    node and at most half the budget, with a non-zero point."""
    import lll_oracle
    import qr_oracle
    B8 = C.bases8()
    assert B8["raw"].shape == (9, 8, 8) and B8["reduced"].shape == (9, 8, 8) and B8["targets"].shape == (9, 64, 8)
    assert np.array_equal(B8["raw"][0], lll_oracle.bases()["qary8"])
    assert len({b.tobytes() for b in B8["raw"]}) == 9
    for p in range(9):
        o = lll_oracle.lll(B8["raw"][p].tolist(), 0.99)
        assert o["status"] == 0 and o["swaps"] > 0
        assert np.array_equal(np.array(o["basis_out"], dtype=np.float64), B8["reduced"][p])
        r = qr_oracle.solve(B8["reduced"][p], B8["targets"][p], max_nodes=C.MAX_NODES)
        assert r["qr_status"] == 0 and not r["status"].any()
        assert (r["nodes"] > 1).all() and (r["nodes"] <= C.MAX_NODES // 2).all() and r["z"].any(axis=1).all()
    assert (B8["sigma"] > 0).all() and len(set(B8["sigma"][:2])) == 2


def test_wang_ling_rejections_on_the_oracle(oracle):
    """Where the probes can ask for 0 < accepts < all.  int12 at the subject's sigma (45, the
    one tests/test_gpu_imhk_targets.py uses for it): the Wang-Ling weights of 64 chains are
    3e-7 apart and every one of 512 proposals is accepted, so lgs_imhk's probes carry in
    unbeatable states for their rejections and lgs_imhk_targets' probe asks for accepts only.
    klein_ntru128 (the pipelined case) and the d = 8 batch (lgs_imhk_bases) reject on their own."""
    import imhkb_oracle
    s = C.subject()
    r = oracle.imhk(s["R"], s["cprime"], s["B"], s["sigma"], 64, C.IMHK_STEPS, seed=C.SEED, first_chain=2,
                    mode=oracle.IMHK_WANG_LING)
    assert int(r["accepts"].sum()) == 64 * C.IMHK_STEPS and np.ptp(r["lw"]) < 1e-6 and r["z"].any()
    s = C.subject("ntru128")
    r = oracle.imhk(s["R"], s["cprime"], s["B"], s["sigma"], 64, C.IMHK_STEPS, seed=C.SEED, first_chain=2,
                    mode=oracle.IMHK_WANG_LING)
    assert 0 < int(r["accepts"].sum()) < 64 * C.IMHK_STEPS
    B8 = C.bases8()
    acc = sum(int(imhkb_oracle.solve(B8["reduced"][p], B8["targets"][p, :3], B8["sigma"][p], 4, 6, C.SEED,
                                     19 + p * 12)["accepts"].sum()) for p in range(2))
    assert 0 < acc < 2 * 3 * 4 * 6


def test_diagnostics_inputs_are_not_degenerate():
    for size in C.SIZES.values():
        x = C.diag_data(size["ns"])
        assert x.shape == (size["ns"], 12) and x.dtype == np.int32
        assert (x.max(0) > x.min(0)).all() and np.abs(x).max() < 32639
