"""Case table of tests/test_gpu_imhk_matrix.py, importable without a GPU.

lgs_imhk / lgs_imhk_trace (the calls Context.imhk makes) in every LGS_CTX_* option, both
weight modes, both store widths, both layouts, both pointer kinds, and the call shapes that
cross a block, a thinning or a chain-counter boundary.  The table is an explicit list, not
the cross product; tests/test_imhk_matrix_host.py checks what it must contain and the
premises of every case on the oracle alone.

Also here: the per-step oracle (per_step_oracle), the reference of `accepted`,
`logw_samples` and the state_init rule, which a whole-call oracle run does not give.
"""
import collections

import numpy as np

SEED = 611  # (IMHK_SEED of test_gpu_kernel_matrix: its bases reject and accept at this seed)

# One max_proposals for every context: the block length is T = max_proposals / n_chains,
# rounded down to a multiple of thin by the library.  300 / 37 = 8, 300 / 64 = 4,
# 300 / 69 = 4, 300 / 256 = 1: none a multiple of thin = 3, and every call below takes at
# least three blocks.
MAX_PROPOSALS = 300

# ------------------------------------------------------------------ contexts
# name -> Context(...) keywords.  hooks (liblgs_hip_hooks.so) is a library choice, not an
# LGS_CTX_* option; max_proposals is the block size above.
CONTEXTS = {
    "default": {},
    "panel16": {"panel": 16},
    "far_fp64": {"far": "fp64"},
    "samplez_libm": {"samplez_libm": True},
    "store32": {"store32": True},
    "panel16+samplez_libm": {"panel": 16, "samplez_libm": True},
    "no_qskip": {"qskip": False},
    "no_pipeline+no_lookahead": {"pipeline": False, "lookahead": False},
}
# The options whose Klein launch leaves something else behind for the accept pass, the
# moments pass, the gathers and B z: crossed with both weight modes on the d = 40 and the
# d = 100 bases.
STORE_CONTEXTS = ("panel16", "far_fp64", "samplez_libm", "store32", "panel16+samplez_libm")
# These two change which launches a device-pointer call on a caller's stream makes and skips
# (include/lgs.h lgs_set_stream); tests/test_gpu_stream.py owns that ground: one case each.
STREAM_CONTEXTS = ("no_qskip", "no_pipeline+no_lookahead")
# Context.__init__ keyword -> the value that turns its LGS_CTX_* option on.  LGS_CTX_NO_CU_SPLIT
# only moves pipelined Klein launches between streams (tests/test_gpu_qskip_clean.py and
# tests/test_gpu_bz_lean.py run it through the hooks build's forced split); it has no case here.
OPTION_ON = {"pipeline": False, "lookahead": False, "samplez_libm": True, "panel": 16, "far": "fp64",
             "store32": True, "qskip": False}
NOT_IN_TABLE = {"cu_split"}
NOT_OPTIONS = {"device", "max_proposals", "hooks"}

# ------------------------------------------------------------------ bases
# name -> why it is here
BASES = {
    "r40": "test_gpu_kernel_matrix._ragged(40) at IMHK_SIGMA: d % 16 = 8, below 64",
    "r130": "_ragged(130) at IMHK_SIGMA: d > 128, a 2-row bottom panel under four (eight) full ones",
    "r100": "_ragged(100) at IMHK_SIGMA: the d = 100 basis of the reference-weight cases",
    "skip100": "_skip(False), d = 100, B = R, centre off 0: speculative sub-panels and a q-panel the reference-mode "
               "kernel skips; the d = 100 basis of the Wang-Ling cases (20 % acceptance) and of the two stream options",
    "kinds100": "_kinds_basis(), d = 100, R only: every SampleZ kind; Wang-Ling weights only (its reference-mode "
                "weights cancel terms of 1e21, test_samplez_kinds_precision_linear_every_kernel)",
    "wide40": "test_gpu_edges._int_basis(40, 5) at sigma 3: the basis of "
              "test_imhk_16bit_store_with_wide_carried_states",
}
_bases = {}


def basis(oracle, name):
    """(R, c', B or None, sigma), shared and read-only."""
    if name not in _bases:
        import test_gpu_kernel_matrix as km
        if name in ("r40", "r100", "r130"):
            R, cp, B, _ = km._ragged(oracle, int(name[1:]))[0]
            b = (R, cp, B, km.IMHK_SIGMA)
        elif name == "skip100":
            b = km._skip(oracle, False)[0]
        elif name == "kinds100":
            R, cp = km._kinds_basis()
            b = (R, cp, None, km.KINDS_SIGMA)
        else:
            from test_gpu_edges import _int_basis
            B = _int_basis(40, 5)
            R, cp = oracle.qr_prepare(B)
            b = (R, cp, B, 3.0)
        for a in b[:3]:
            if a is not None:
                a.setflags(write=False)
        _bases[name] = b
    return _bases[name]


def centre(oracle, name):
    """The lattice-frame centre c of the basis's c' = Q^T c, which the oracle's reference-mode
    weight reads: 0 but for skip100, whose B = R makes Q the identity and c = c'."""
    R, cp, B, _ = basis(oracle, name)
    if name == "skip100":
        assert B is R
        return cp
    assert not cp.any() or B is None
    return None


# ------------------------------------------------------------------ call shapes
Shape = collections.namedtuple("Shape", "nc steps thin first_chain split")
# (n_chains, n_steps, thin, first_chain, split): split lists the consecutive calls, each
# continuing first_step; every part but the last is a multiple of thin, so the kept states of
# the sequence are those of the single call.
SHAPES = {
    # 64 chains: T = 3 (192 proposals: the fp64-far-field MFMA kernel), blocks 3 3 3 3 3 3 2,
    # 20 % 3 = 2 steps behind the last kept state
    "c64": Shape(64, 20, 3, 0, (20,)),
    "c64-split": Shape(64, 20, 3, 0, (9, 11)),          # 3 and 4 blocks
    "c64-first5": Shape(64, 20, 3, 5, (20,)),           # rows 5.. of c69
    "c69": Shape(69, 20, 3, 0, (20,)),                  # (276 proposals: the VALU kernel)
    # thin 1, T = 4: 256 proposals, one workgroup of the int8-digit kernel; blocks 4 4 4 4 1
    "c64-thin1": Shape(64, 17, 1, 0, (17,)),
    # 256 chains: T = 1, 17 blocks of one workgroup each
    "c256-thin1": Shape(256, 17, 1, 0, (17,)),
    # T = 3: 768 proposals, three workgroups; the last block has 2 steps (512)
    "c256": Shape(256, 20, 3, 0, (20,)),
    # 37 chains up to the last chain counter: T = 6 (222 proposals: VALU), blocks 6 6 6 5
    "c37-top": Shape(37, 23, 3, 2 ** 32 - 37, (23,)),
    "c37-top-split": Shape(37, 23, 3, 2 ** 32 - 37, (18, 5)),   # 3 blocks and 1
}
FIRST_STEP = 1


def block_length(shape):
    """The library's block: max_proposals / n_chains, rounded down to a multiple of thin
    (csrc/lgs_capi.hip imhk_impl)."""
    q = max(1, MAX_PROPOSALS // shape.nc)
    if q < shape.steps:
        q = max(shape.thin, q // shape.thin * shape.thin)
    return q


# ------------------------------------------------------------------ cases
# init: None = chains start uninitialised; "set" = a caller-set state (state_init = 1) with
# its Wang-Ling weight; "wide" = the same with coefficients beyond int16
# stream: device pointers on a caller's stream (the early check, pipelined blocks)
Case = collections.namedtuple("Case", "ctx basis wl z64 cm dev shape init stream")


def case_id(c):
    return "-".join([c.ctx, c.basis, "wl" if c.wl else "ref", "z64" if c.z64 else "z32", "cm" if c.cm else "rm",
                     ("stream" if c.stream else "dev") if c.dev else "host", c.shape] + ([c.init] if c.init else []))


def _c(ctx, basis, wl, shape, z64=False, cm=False, dev=False, init=None, stream=False):
    return Case(ctx, basis, bool(wl), z64, cm, dev, shape, init, stream)


def _build():
    out = []
    # 1. every store option x both weight modes x the d = 40 and d = 100 bases (d = 100:
    #    reference weights on r100, Wang-Ling on skip100 and kinds100), at 64 chains
    #    (fp64-far-field MFMA kernel, thin 3) and at 256 chains (int8-digit kernel, thin 1)
    for ctx in ("default",) + STORE_CONTEXTS:
        for b, wl in (("r40", False), ("r40", True), ("r100", False), ("skip100", True), ("kinds100", True)):
            out += [_c(ctx, b, wl, "c64"), _c(ctx, b, wl, "c256-thin1")]
        # d = 130: every chain of c64 against the oracle, every 4th of c256
        for wl in (False, True):
            out.append(_c(ctx, "r130", wl, "c64"))
    for ctx in ("default", "panel16", "store32"):
        out.append(_c(ctx, "r130", True, "c256"))
    # 2. store width, layout, pointer kind: all eight on the default context (d = 40, both
    #    modes on half of them), pairs on the store options
    for z64 in (False, True):
        for cm in (False, True):
            for dev in (False, True):
                if z64 or cm or dev:
                    out.append(_c("default", "r40", True, "c64", z64, cm, dev))
                    if z64 != cm:
                        out.append(_c("default", "r40", False, "c64", z64, cm, dev))
    out += [_c("default", "skip100", True, "c256-thin1", z64=True, cm=True, dev=True),
            _c("default", "r130", True, "c64", dev=True),
            _c("store32", "r40", True, "c64", z64=True), _c("store32", "r40", True, "c64", cm=True, dev=True),
            _c("store32", "skip100", True, "c256-thin1", dev=True),
            _c("panel16", "r40", True, "c64", cm=True, dev=True), _c("panel16", "r40", True, "c64", z64=True, dev=True),
            _c("panel16", "skip100", False, "c256-thin1", z64=True, cm=True),
            _c("far_fp64", "r40", True, "c64", z64=True, dev=True), _c("far_fp64", "skip100", True, "c256-thin1", cm=True),
            _c("samplez_libm", "kinds100", True, "c64", z64=True, cm=True),
            _c("samplez_libm", "r40", True, "c64", dev=True),
            _c("panel16+samplez_libm", "kinds100", True, "c256-thin1", z64=True),
            _c("panel16+samplez_libm", "r40", False, "c64", cm=True, dev=True)]
    # 3. call shapes: split calls, first_chain 5 against the 69-chain run, the top of the
    #    chain counter, one workgroup of the int8-digit kernel, three workgroups
    for b, wl in (("r40", False), ("r40", True), ("r100", False), ("skip100", True)):
        for s in ("c64-split", "c64-first5", "c69", "c64-thin1", "c37-top", "c37-top-split", "c256"):
            out.append(_c("default", b, wl, s))
    for ctx in ("panel16", "store32", "samplez_libm"):
        out += [_c(ctx, "r40", True, "c64-split", dev=True), _c(ctx, "r40", True, "c37-top"),
                _c(ctx, "skip100", True, "c64-thin1")]
    # 4. reference weights around a centre off 0, and the two stream options: reference weights (the early check), device pointers on a
    #    caller's stream, on the basis with a q-panel to skip; the default context beside them
    for ctx in ("default", "panel16", "store32"):
        out.append(_c(ctx, "skip100", False, "c256-thin1"))
    out.append(_c("default", "skip100", False, "c256-thin1", dev=True, stream=True))
    for ctx in STREAM_CONTEXTS:
        out.append(_c(ctx, "skip100", False, "c256-thin1", dev=True, stream=True))
    # 5. a caller-set state under Wang-Ling
    for ctx in ("default", "panel16", "samplez_libm", "store32", "far_fp64"):
        out.append(_c(ctx, "r40", True, "c64", init="set"))
    out += [_c("default", "r40", True, "c64", dev=True, init="set"),
            _c("default", "r40", True, "c64-split", cm=True, dev=True, init="set")]
    # 6. carried states beyond int16: the default store widens in its first block, store32 does not
    for ctx in ("default", "store32"):
        out += [_c(ctx, "wide40", True, "c64", dev=True, init="wide"), _c(ctx, "wide40", True, "c64", init="wide")]
    assert len(set(out)) == len(out)
    return tuple(out)


CASES = _build()
CASE_IDS = tuple(case_id(c) for c in CASES)
# forced resolution: Context(panel=16, hooks=True) with every Wang-Ling bound widened
FORCED = _c("panel16", "r40", True, "c64")
FORCED_SCALES = (3e3, 1e16)


def group_key(c):
    """Cases of one key are the same chains: every output equals the key's base case."""
    return (c.basis, c.wl, SHAPES[c.shape].nc, SHAPES[c.shape].steps, SHAPES[c.shape].thin,
            SHAPES[c.shape].first_chain, c.init)


def base_case(key):
    """The default context, host pointers, int32, row-major, one call."""
    for c in CASES:
        if (group_key(c) == key and c.ctx == "default" and not (c.z64 or c.cm or c.dev) and
                len(SHAPES[c.shape].split) == 1):
            return c
    raise KeyError(key)


GROUPS = tuple(sorted({group_key(c) for c in CASES}, key=str))


def oracle_rows(c):
    """The chains compared with the oracle: every one, but every 4th at d = 130 with more
    than 64 chains."""
    nc = SHAPES[c.shape].nc
    return range(0, nc, 4) if c.basis == "r130" and nc > 64 else range(nc)


# ------------------------------------------------------------------ caller-set states
WIDE_LW_ADVANTAGE = 3.0


def initial_state(oracle, c):
    """None, or (z, lw) of a caller-set state: lattice points a few sigma_i off the centre
    with their Wang-Ling weights; "wide": column 0 at 50000 and one -70000, as
    test_imhk_16bit_store_with_wide_carried_states sets them, with WIDE_LW_ADVANTAGE on top of
    their weights (that test's 1e6 keeps every state for ever; exp(-3) a step lets a third of the
    chains move within the call, so kept states mix carried wide states and proposals)."""
    if c.init is None:
        return None
    R, cp, B, sigma = basis(oracle, c.basis)
    nc, d = SHAPES[c.shape].nc, R.shape[0]
    z = np.random.default_rng(1).integers(-5, 6, (nc, d)).astype(np.int64)
    if c.init == "wide":
        z[:, 0] = 50000
        z[3, 5] = -70000
    lw = np.array([oracle.log_weight(R, cp, B, sigma, z[k], mode=oracle.IMHK_WANG_LING) for k in range(nc)])
    if c.init == "wide":
        lw += WIDE_LW_ADVANTAGE
    return z, lw


# ------------------------------------------------------------------ the per-step oracle
_oracle_runs = {}


def per_step_oracle(oracle, R, cp, B, sigma, nc, steps, *, seed, first_chain, first_step, wl, state=None,
                    center=None):
    """lgs_oracle.imhk one step at a time (n_steps = 1, resuming `state`) for steps
    first_step .. first_step + steps - 1.  Returns dict(states nc x steps x d, lw nc x steps
    (the log weight after each step), accepted nc x steps (the increase of accepts), and the
    final z, lw, accepts)."""
    d = R.shape[0]
    Bo = B if B is not None else np.zeros_like(R)  # (Wang-Ling weights do not read B)
    mode = oracle.IMHK_WANG_LING if wl else oracle.IMHK_REFERENCE
    st = None
    if state is not None:
        st = {"z": np.array(state[0], dtype=np.int64), "lw": np.array(state[1], dtype=np.float64),
              "init": np.ones(nc, dtype=np.int32), "accepts": np.zeros(nc, dtype=np.int64)}
    states = np.zeros((nc, steps, d), dtype=np.int64)
    lw = np.zeros((nc, steps))
    accepted = np.zeros((nc, steps), dtype=np.uint8)
    prev = np.zeros(nc, dtype=np.int64)
    for t in range(steps):
        st = oracle.imhk(R, cp, Bo, sigma, nc, 1, center=center, seed=seed, first_chain=first_chain,
                         first_step=first_step + t, state=st, mode=mode)
        st = {k: st[k] for k in ("z", "lw", "init", "accepts")}
        states[:, t] = st["z"]
        lw[:, t] = st["lw"]
        accepted[:, t] = st["accepts"] - prev
        prev = st["accepts"].copy()
    return {"states": states, "lw": lw, "accepted": accepted, "z": st["z"].copy(), "lw_final": st["lw"].copy(),
            "accepts": st["accepts"].copy()}


def case_oracle(oracle, c):
    """The per-step oracle of a case's chains (oracle_rows), cached by what decides them."""
    rows = oracle_rows(c)
    key = group_key(c) + (rows.step,)
    if key not in _oracle_runs:
        R, cp, B, sigma = basis(oracle, c.basis)
        s = SHAPES[c.shape]
        init = initial_state(oracle, c)
        kw = dict(seed=SEED, first_step=FIRST_STEP, wl=c.wl, center=centre(oracle, c.basis))
        if rows.step == 1:
            o = per_step_oracle(oracle, R, cp, B, sigma, s.nc, s.steps, first_chain=s.first_chain, state=init, **kw)
        else:  # chain by chain
            parts = [per_step_oracle(oracle, R, cp, B, sigma, 1, s.steps, first_chain=s.first_chain + k,
                                     state=None if init is None else (init[0][k:k + 1], init[1][k:k + 1]), **kw)
                     for k in rows]
            o = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        for a in o.values():
            a.setflags(write=False)
        _oracle_runs[key] = o
    return _oracle_runs[key]


def expected(c, o):
    """What lgs_imhk returns for the oracle's chains: kept states (steps thin, 2 thin, ...),
    their log weights, the integer moments over them, and the state_init words: the step of
    the chain's last accepted proposal + 2 (2 after the initial draw alone; 1 for a
    caller-set state no proposal replaced)."""
    s = SHAPES[c.shape]
    kept = o["states"][:, s.thin - 1::s.thin]
    assert kept.shape[1] == s.steps // s.thin
    flat = kept.reshape(-1, kept.shape[2])
    last = np.where(o["accepted"].any(axis=1), s.steps - 1 - np.argmax(o["accepted"][:, ::-1], axis=1) + FIRST_STEP, 0)
    init = np.where(last > 0, last + 2, 2 if c.init is None else 1).astype(np.int32)
    return {"kept": kept, "lw_kept": o["lw"][:, s.thin - 1::s.thin],
            "moments": np.concatenate([flat.sum(0), (flat * flat).sum(0)]), "init": init}
