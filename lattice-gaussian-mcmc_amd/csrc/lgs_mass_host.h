// lgs_mass_host.h -- the host's part of lgs_gaussian_mass (include/lgs.h):
// splitting every target's enumeration tree into independent work items, and combining
// the items' results per target.  Plain C++, no HIP: tests/test_mass_host.py compiles it
// into a stand-alone program.  Compile with -ffp-contract=off: the walk below is the
// operational definition of lgs.h, one rounding per operation, as the kernel's.
//
// The radius of lgs_gaussian_mass never shrinks, so the subtree below a node does not depend
// on any other subtree.  The host walks the top k levels (d-1 .. d-k) of every tree exactly
// as the unsplit traversal would, counts the nodes it visits there, and emits one item per
// node of level top = d - k with P < A: the prefix z[top .. d-1] and P[top].  An item's lane
// starts on level top - 1 and visits the nodes the unsplit traversal visits below that node,
// so host nodes + the items' nodes are the nodes of the unsplit traversal, and the points
// are the same points.
//
// The walk is level by level: the items of depth k + 1 are the children of the items of
// depth k, each parent's children in zig-zag order until the first with P >= A (which the
// unsplit traversal visits too, and prunes), parents in their own order -- the order of the
// depth-first traversal restricted to that level.  No level is walked twice.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

namespace lgs {
namespace mass_host {

constexpr int64_t kItemsWanted = 1 << 14;  // deepen until the call has this many items
constexpr int64_t kItemsMax = 1 << 18;     // never more items than this
constexpr int64_t kWalkMax = 1 << 20;      // nodes the host walks at most
constexpr double kMaxAbsZ = 4503599627370496.0;  // 2^52, as the kernel's kCvpMaxAbsZ

struct Split {
    int d = 0, k = 0, top = 0;
    int64_t n = 0;                    // targets
    int64_t items = 0;
    bool nonfinite = false;           // a target or a conditional mean of the walk was not finite
    std::vector<int32_t> tgt;         // items: the item's target (ascending)
    std::vector<double> z;            // k x items: z[top + r] of item q at [r * items + q]
    std::vector<double> P;            // items: P[top]
    std::vector<int64_t> host_nodes;  // n: nodes of levels >= top
};

// The items of one depth while the split deepens, item-major: row q = z[top .. d-1].
struct Level {
    int k = 0;
    std::vector<int32_t> tgt;
    std::vector<double> rows, P;
    std::vector<int64_t> host_nodes;
    int64_t nodes = 0;  // sum of host_nodes
    int64_t items() const { return (int64_t)tgt.size(); }
};

// The children of cur's items: level top - 1 = d - cur.k - 1.  cp: c' coordinate-major,
// element i of target t at cp[i * ldc + t].  false once the walk has passed node_cap nodes
// in all or item_cap items (next is then incomplete); a non-finite target or conditional mean
// sets nonfinite and ends the walk.
inline bool deepen(const double* R, int d, const double* cp, int64_t ldc, const double* radius2, const Level& cur,
                   int64_t node_cap, int64_t item_cap, Level& next, bool& nonfinite) {
    const int k = cur.k, i = d - k - 1;
    next.k = k + 1;
    next.tgt.clear();
    next.rows.clear();
    next.P.clear();
    next.host_nodes = cur.host_nodes;
    next.nodes = cur.nodes;
    const double* Ri = R + (size_t)i * d;
    const int64_t m = cur.items();
    for (int64_t q = 0; q < m; ++q) {
        const int64_t t = cur.tgt[(size_t)q];
        const double* zq = cur.rows.data() + (size_t)q * k;  // z[i+1 .. d-1]
        const double A = radius2[t];
        if (k == 0)
            for (int j = 0; j < d; ++j)
                if (!std::isfinite(cp[(size_t)j * ldc + t])) {
                    nonfinite = true;
                    return true;
                }
        double cs = 0.0;
        for (int j = i + 1; j < d; ++j) cs = cs + Ri[j] * zq[j - i - 1];
        const double base = cp[(size_t)i * ldc + t] - cs;
        const double mean = base / Ri[i];
        double z = std::rint(mean);
        if (!(std::fabs(mean) < kMaxAbsZ)) {
            nonfinite = true;
            return true;
        }
        double sn = mean >= z ? 1.0 : -1.0;
        for (;;) {
            ++next.host_nodes[(size_t)t];
            if (++next.nodes > node_cap) return false;
            const double r = base - Ri[i] * z;
            const double Pi = cur.P[(size_t)q] + r * r;
            if (!(Pi < A)) break;  // every further sibling is farther
            if (next.items() >= item_cap) return false;
            next.tgt.push_back((int32_t)t);
            next.rows.push_back(z);
            next.rows.insert(next.rows.end(), zq, zq + k);
            next.P.push_back(Pi);
            z += sn;
            sn = -(sn + (sn > 0.0 ? 1.0 : -1.0));
        }
    }
    return true;
}

// The items of a chunk of n targets (of a call of n_call).  k >= 0: that depth (<= d - 1).
// k < 0, the rule: deepen level by level until the chunk has kItemsWanted items (or none at
// all), k = d - 1, the next level would have more than kItemsMax items, or the walk would pass
// kWalkMax nodes; k = 0, the unsplit trees (R and cp are not read), when the call alone has
// kItemsWanted targets.
inline Split split(const double* R, int d, int64_t n, int64_t n_call, const double* cp, int64_t ldc,
                   const double* radius2, int k) {
    const int64_t none = std::numeric_limits<int64_t>::max();
    Level cur, next;
    cur.tgt.resize((size_t)n);
    for (int64_t t = 0; t < n; ++t) cur.tgt[(size_t)t] = (int32_t)t;
    cur.P.assign((size_t)n, 0.0);
    cur.host_nodes.assign((size_t)n, 0);
    bool nonfinite = false;
    if (k >= 0) {
        while (cur.k < k && cur.k < d - 1 && !nonfinite) {
            deepen(R, d, cp, ldc, radius2, cur, none, none, next, nonfinite);
            std::swap(cur, next);
        }
    } else if (n_call < kItemsWanted) {
        while (cur.items() > 0 && cur.items() < kItemsWanted && cur.k < d - 1) {
            if (!deepen(R, d, cp, ldc, radius2, cur, kWalkMax, kItemsMax, next, nonfinite)) break;
            std::swap(cur, next);
            if (nonfinite) break;
        }
    }
    Split s;
    s.d = d;
    s.k = cur.k;
    s.top = d - cur.k;
    s.n = n;
    s.items = cur.items();
    s.nonfinite = nonfinite;
    s.tgt = std::move(cur.tgt);
    s.P = std::move(cur.P);
    s.host_nodes = std::move(cur.host_nodes);
    s.z.resize((size_t)s.items * s.k);
    for (int64_t q = 0; q < s.items; ++q)
        for (int r = 0; r < s.k; ++r) s.z[(size_t)r * s.items + q] = cur.rows[(size_t)q * s.k + r];
    return s;
}

struct ItemResults {   // per item, as the kernel leaves them
    const double *mass, *energy, *dmin;
    const int64_t *points, *nodes;
    const int32_t* status;
    const double* sz;  // nullable: d x ldo, S[j] of item q at [j * ldo + q], rows >= top unused
    int64_t ldo;
};
struct TargetResults {  // per target, every array of n (sum_z: n x d row-major, nullable)
    double *mass, *energy, *dmin, *sum_z;
    int64_t *points, *nodes;
    int32_t* status;
};

// Sums the items of every target.  nodes: the host's plus the items'; status 1 when an item
// stopped at its budget or the total exceeds max_nodes -- either way the complete traversal
// has more than max_nodes nodes -- and nodes is then max_nodes, as the unsplit search reports.
// S[j] of the prefix levels j >= top: z_j of the item times the item's mass (the msub rule,
// with the item's mass as msub[top]).
inline void combine(const Split& s, int64_t max_nodes, const ItemResults& r, const TargetResults& o) {
    const int d = s.d;
    for (int64_t t = 0; t < s.n; ++t) {
        o.mass[t] = 0.0;
        o.energy[t] = 0.0;
        o.dmin[t] = std::numeric_limits<double>::infinity();
        o.points[t] = 0;
        o.nodes[t] = s.host_nodes[(size_t)t];
        o.status[t] = 0;
        if (o.sum_z)
            for (int j = 0; j < d; ++j) o.sum_z[(size_t)t * d + j] = 0.0;
    }
    for (int64_t q = 0; q < s.items; ++q) {
        const int64_t t = s.tgt[(size_t)q];
        o.mass[t] = o.mass[t] + r.mass[q];
        o.energy[t] = o.energy[t] + r.energy[q];
        o.dmin[t] = std::min(o.dmin[t], r.dmin[q]);
        o.points[t] += r.points[q];
        o.nodes[t] += r.nodes[q];
        if (r.status[q] != 0) o.status[t] = 1;
        if (o.sum_z && r.sz) {
            double* S = o.sum_z + (size_t)t * d;
            for (int j = 0; j < s.top; ++j) S[j] = S[j] + r.sz[(size_t)j * r.ldo + q];
            for (int j = s.top; j < d; ++j) S[j] = S[j] + s.z[(size_t)(j - s.top) * s.items + q] * r.mass[q];
        }
    }
    for (int64_t t = 0; t < s.n; ++t) {
        if (o.nodes[t] > max_nodes) o.status[t] = 1;
        if (o.status[t]) o.nodes[t] = max_nodes;
    }
}

}  // namespace mass_host
}  // namespace lgs
