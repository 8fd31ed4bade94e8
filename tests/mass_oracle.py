"""CPU oracle of the exact Gaussian mass (lgs_gaussian_mass): a transcription, in pure Python
floats (IEEE fp64, one rounding per operation), of the fixed-radius traversal that
include/lgs.h defines -- lgs_closest_vector's loop with a bound that never shrinks and a
weight on every leaf -- with the msub rule for sum_z.  Run on the c' a library
call reports, points, nodes, status and dist2_min compare bit for bit; the three sums are
defined up to the order of summation and compare within tolerances().  Also the partial-tree
work items of the split (top, prefix, P_top), a transcription of the host's walk of the top
levels, and a brute-force box sum."""
import itertools
import math

import numpy as np

from cvp_oracle import qr, refdist, setup  # noqa: F401  (the tests take bases and targets from there)

U52 = 2.0 ** -52
TINY = 2.3e-308  # a flushed subnormal term


def enum(R, cp, sigma, radius2, shift=0.0, max_nodes=1 << 40, top=None, prefix=(), P_top=0.0):
    """The traversal of lgs.h below the node (z[top..d-1] = prefix, P[top] = P_top); top = d
    (default): the whole tree.  Returns a dict: mass, energy, points, dist2_min, sum_z (d
    floats; levels >= top are left 0 -- the host forms them from the item's mass), abs_z (A_j =
    sum |z_j| w, the same way), nodes, status."""
    Rl, cpl = np.asarray(R).tolist(), np.asarray(cp).tolist()
    d = len(cpl)
    top = d if top is None else top
    assert 1 <= top <= d and len(prefix) == d - top
    z, base, P, nxt, stp = [0] * d, [0.0] * d, [0.0] * (d + 1), [0] * d, [0] * d
    for j in range(top, d):
        z[j] = int(prefix[j - top])
    P[top] = float(P_top)
    A, sh = float(radius2), float(shift)
    two_s2 = 2.0 * sigma * sigma
    msub, S, Aabs = [0.0] * (d + 1), [0.0] * d, [0.0] * d
    asub = [0.0] * (d + 1)

    def enter(i):
        cs = 0.0
        Ri = Rl[i]
        for j in range(i + 1, d):
            cs = cs + Ri[j] * z[j]
        b = cpl[i] - cs
        m = b / Ri[i]
        z0 = round(m)  # round-half-even
        base[i] = b
        z[i] = z0
        stp[i] = 1 if m >= z0 else -1
        nxt[i] = 0

    mass, energy, points, dmin, nodes, status = 0.0, 0.0, 0, math.inf, 0, 0
    i = top - 1
    enter(i)
    while True:
        if nodes == max_nodes:
            status = 1
            break
        nodes += 1
        r = base[i] - Rl[i][i] * z[i]
        Pi = P[i + 1] + r * r
        if Pi < A:
            if i == 0:
                w = math.exp((sh - Pi) / two_s2)
                points += 1
                dmin = min(dmin, Pi)
                mass = mass + w
                energy = energy + w * Pi
                msub[1] = msub[1] + w
                asub[1] = asub[1] + w
                S[0] = S[0] + z[0] * w
                Aabs[0] = Aabs[0] + abs(z[0]) * w
            else:
                P[i] = Pi
                i -= 1
                enter(i)
                continue
        else:
            i += 1
            if i == top:
                break
            # the subtree below the node being left at level i is complete
            S[i] = S[i] + z[i] * msub[i]
            Aabs[i] = Aabs[i] + abs(z[i]) * asub[i]
            msub[i + 1] = msub[i + 1] + msub[i]
            asub[i + 1] = asub[i + 1] + asub[i]
            msub[i] = asub[i] = 0.0
        nxt[i] += 1
        z[i] += stp[i] * nxt[i]
        stp[i] = -stp[i]
    if status == 1:  # the open subtrees along the path, so that sum_z covers the points visited
        run = 0.0
        for k in range(1, top):
            run = run + msub[k]
            S[k] = S[k] + z[k] * run
            Aabs[k] = Aabs[k] + abs(z[k]) * run
    return dict(mass=mass, energy=energy, points=points, dist2_min=dmin, sum_z=S, abs_z=Aabs, nodes=nodes,
                status=status)


def host_walk(R, cp, radius2, k, node_cap=None, item_cap=None):
    """The host's walk of levels d-1 .. d-k (lgs_mass_host.h): (items, nodes) with items a
    list of (prefix z[top..d-1], P[top]) in traversal order.  k = 0: one item, no nodes.
    With caps: None as soon as the walk passes node_cap nodes or item_cap items."""
    Rl, cpl = np.asarray(R).tolist(), np.asarray(cp).tolist()
    d = len(cpl)
    top = d - k
    if k == 0:
        return [((), 0.0)], 0
    z, base, P, nxt, stp = [0] * d, [0.0] * d, [0.0] * (d + 1), [0] * d, [0] * d
    A = float(radius2)

    def enter(i):
        cs = 0.0
        for j in range(i + 1, d):
            cs = cs + Rl[i][j] * z[j]
        b = cpl[i] - cs
        m = b / Rl[i][i]
        z0 = round(m)
        base[i], z[i], stp[i], nxt[i] = b, z0, (1 if m >= z0 else -1), 0

    items, nodes = [], 0
    i = d - 1
    enter(i)
    while True:
        nodes += 1
        if node_cap is not None and nodes > node_cap:
            return None
        r = base[i] - Rl[i][i] * z[i]
        Pi = P[i + 1] + r * r
        if Pi < A:
            if i == top:
                items.append((tuple(z[top:]), Pi))
                if item_cap is not None and len(items) > item_cap:
                    return None
            else:
                P[i] = Pi
                i -= 1
                enter(i)
                continue
        else:
            i += 1
            if i == d:
                break
        nxt[i] += 1
        z[i] += stp[i] * nxt[i]
        stp[i] = -stp[i]
    return items, nodes


def box_sum(R, cp, sigma, radius2, centre, half, shift=0.0):
    """Brute force over centre + [-half, half]^d: (mass, energy, points, dist2_min, sum_z,
    abs_z) of the points with refdist < radius2, math.fsum-exact sums."""
    two_s2 = 2.0 * sigma * sigma
    d = len(cp)
    ws, es, pts, dmin = [], [], 0, math.inf
    sz, az = [[] for _ in range(d)], [[] for _ in range(d)]
    for off in itertools.product(range(-half, half + 1), repeat=d):
        zz = [int(c) + o for c, o in zip(centre, off)]
        D = refdist(R, cp, zz)
        if D < radius2:
            w = math.exp((shift - D) / two_s2)
            pts += 1
            dmin = min(dmin, D)
            ws.append(w)
            es.append(w * D)
            for j in range(d):
                sz[j].append(w * zz[j])
                az[j].append(w * abs(zz[j]))
    return (math.fsum(ws), math.fsum(es), pts, dmin, [math.fsum(v) for v in sz], [math.fsum(v) for v in az])


def tolerances(N, mass, energy, abs_z):
    """The bounds of the issue, N the target's point count: both sides evaluate
    (shift - Pi) / two_s2 with identical IEEE operations and each exp is within 1 ulp, so a
    term differs by at most 4u relative (u = 2^-53); a sum of N non-negative terms in any order
    is within (N-1)u of its exact value.  Hence mass within (N + 8) 2^-52 relative, energy
    within (N + 10) 2^-52 relative, sum_z[j] within (2N + 16) 2^-52 A_j absolute (the msub
    additions, one product and the signed sum are each bounded through sum |terms| = A_j); each
    plus N 2.3e-308 absolute for flushed subnormals."""
    return ((N + 8) * U52 * mass + N * TINY, (N + 10) * U52 * energy + N * TINY,
            [(2 * N + 16) * U52 * a + N * TINY for a in abs_z])


def close(got, want, N):
    """got / want: dicts with mass, energy, sum_z (want also abs_z); returns the largest ratio
    of |difference| to its tolerance (<= 1 passes).  sum_z of got may be None."""
    tm, te, tz = tolerances(N, want["mass"], want["energy"], want["abs_z"])
    ratios = [abs(got["mass"] - want["mass"]) / tm if tm else float(got["mass"] != want["mass"]),
              abs(got["energy"] - want["energy"]) / te if te else float(got["energy"] != want["energy"])]
    if got.get("sum_z") is not None:
        for g, w, t in zip(got["sum_z"], want["sum_z"], tz):
            ratios.append(abs(g - w) / t if t else float(g != w))
    return max(ratios)
