"""What a range list must be, in plain numpy: no oracle, no GPU.

A decomposition (ZN.zranges, XZ2SFC.ranges, XZ3SFC.ranges) is free in how fine its ranges are; what it
may not do is miss a key that matches, call `contained` a range that holds a key that does not, or
leave the list unsorted or unmerged.  The checkers here state exactly that over a universe small enough
to enumerate, and return the violations they find as [(kind, [first offenders])] -- an empty list is
a pass -- so that an assert message names the z or the code.

Properties that the reference does NOT have, and that are therefore not checked:
  * a merged Z list is not bounded by maxRanges: the budget stops the walk (ZN.scala:214) but bottomOut
    (ZN.scala:173-180) then adds the rest of the queue, and 51 ranges for 50 or 4 for 1 come out;
  * an XZ list is not tight: level g is never classified (`while (level < g ...)`, XZ2SFC.scala:205,
    XZ3SFC.scala:215) and a full sequence interval (XZ2SFC.scala:297-309) runs up to the next sibling's
    code, so the list holds codes of elements that meet no window.  Cover and soundness are one-sided.

"contained" after the merge.  The same full interval makes X3 hold for the XZ curves only vacuously: a
contained element E gives [code(E), code(F)], where F is the element with the next code after E's subtree
-- E's next sibling, or the next sibling of the ancestor A that E is the last descendant of.  E's
enlarged cell reaches half of E's width past A's upper faces and F's enlarged cell, twice F's width,
reaches back over them, so the two intersect: F meets every window that contains E.  F is then in the
list as well, as an overlapping element's [code(F), code(F)] or, past the budget, as a bottomed-out full
interval (XZ2SFC.scala:219-227), unless it is contained too and the argument repeats; the chain ends at
the curve's last element, whose enlarged cell leaves the unit cube and is never contained.  The merge
(XZ2SFC.scala:231-249) joins E's range to F's and ands the flags, so no range of a merged XZ list is
`contained`.  The XZ tests therefore cannot ask for a `contained` range in their inputs; that X3 sees a
wrong flag is shown by the checker's self-test, and the flag itself is held to the oracle's by the
parity tests.
"""
import numpy as np

FIRST = 5   # offenders reported per kind


def as_arrays(ranges):
    """(lower, upper, contained) int64 / int64 / bool arrays of a list of (lower, upper, contained)
    triples or of a structured array with those fields."""
    if isinstance(ranges, np.ndarray) and ranges.dtype.names:
        return (ranges["lower"].astype(np.int64), ranges["upper"].astype(np.int64), ranges["contained"].astype(bool))
    rows = [(int(r[0]), int(r[1]), bool(r[2])) for r in ranges]
    lo = np.array([r[0] for r in rows], np.int64)
    hi = np.array([r[1] for r in rows], np.int64)
    return lo, hi, np.array([r[2] for r in rows], bool)


# ---------------------------------------------------------------- bit interleaving
def interleave(dims):
    """z of per-dimension values (sequence of D int64 arrays, D = 2 or 3): bit i of dimension d is bit
    D * i + d of z (Z2.scala:53, Z3.scala:66-68)."""
    D = len(dims)
    nbits = 31 if D == 2 else 21
    z = np.zeros(np.shape(dims[0]), np.int64)
    for d in range(D):
        v = np.asarray(dims[d], np.int64)
        for i in range(nbits):
            z |= ((v >> i) & 1) << (D * i + d)
    return z


def deinterleave(z, D):
    """The D per-dimension values of z, as a list of int64 arrays."""
    z = np.asarray(z, np.int64)
    nbits = 31 if D == 2 else 21
    out = []
    for d in range(D):
        v = np.zeros(z.shape, np.int64)
        for i in range(nbits):
            v |= ((z >> (D * i + d)) & 1) << i
        out.append(v)
    return out


def z_universe(D, bits, prefix=0):
    """Every z = prefix | [0, 2^(D * bits)), ascending, with its per-dimension values (prefix bits
    included).  prefix has no bit below D * bits."""
    n = 1 << (D * bits)
    assert prefix & (n - 1) == 0
    z = np.int64(prefix) + np.arange(n, dtype=np.int64)
    return z, deinterleave(z, D)


def _covered(lo, hi, z0, n):
    """Mask over the universe slots [z0, z0 + n): the slot lies in some range."""
    a = np.clip(lo - z0, 0, n)
    b = np.clip(hi - z0 + 1, 0, n)
    keep = b > a
    d = np.zeros(n + 1, np.int64)
    np.add.at(d, a[keep], 1)
    np.add.at(d, b[keep], -1)
    return np.cumsum(d[:n]) > 0


def _order_violations(lo, hi, out):
    """Z1 / X1: lower <= upper, ascending and disjoint, and merged (no range starts at previous upper + 1)."""
    bad = np.nonzero(lo > hi)[0]
    if len(bad):
        out.append(("inverted", [(int(lo[i]), int(hi[i])) for i in bad[:FIRST]]))
    if len(lo) > 1:
        bad = np.nonzero(lo[1:] <= hi[:-1])[0]
        if len(bad):
            out.append(("order", [(int(hi[i]), int(lo[i + 1])) for i in bad[:FIRST]]))
        bad = np.nonzero(lo[1:] == hi[:-1] + 1)[0]
        if len(bad):
            out.append(("unmerged", [(int(hi[i]), int(lo[i + 1])) for i in bad[:FIRST]]))


def z_inside(dims, bounds, D):
    """Mask over the universe: the z's dimensions lie inside some bound, dimension by dimension, closed
    (Z3.contains / Z2.contains on every dimension: Z3.scala:93-98, Z2.scala:80-83).  bounds = [(zmin, zmax)]."""
    inside = np.zeros(dims[0].shape, bool)
    for (zmin, zmax) in bounds:
        lo = deinterleave(np.int64(zmin), D)
        hi = deinterleave(np.int64(zmax), D)
        ok = np.ones(dims[0].shape, bool)
        for d in range(D):
            ok &= (dims[d] >= lo[d]) & (dims[d] <= hi[d])
        inside |= ok
    return inside


def check_z_list(ranges, bounds, D, bits, prefix=0, exact=False, universe=None):
    """A ZN.zranges list (range precision 64) for raw (zmin, zmax) bounds inside the universe
    prefix | [0, 2^(D * bits)):
      Z1  lower <= upper, ascending, each lower > previous upper + 1            "inverted" "order" "unmerged"
      Z2  every range inside the universe                                       "outside"
      Z3  every z inside some bound is in a range                               "cover"
      Z4  every z of a `contained` range is inside some bound                   "soundness"
      Z5  (exact: maxRanges None, maxRecurse >= levels) covered set == inside set, all `contained`
                                                                                "exact" "not-contained"
    """
    lo, hi, cont = as_arrays(ranges)
    z, dims = universe if universe is not None else z_universe(D, bits, prefix)
    n = len(z)
    z0 = int(z[0])
    out = []
    _order_violations(lo, hi, out)
    bad = np.nonzero((lo < z0) | (hi > z0 + n - 1))[0]
    if len(bad):
        out.append(("outside", [(int(lo[i]), int(hi[i])) for i in bad[:FIRST]]))
    inside = z_inside(dims, bounds, D)
    cov = _covered(lo, hi, z0, n)
    bad = np.nonzero(inside & ~cov)[0]
    if len(bad):
        out.append(("cover", [int(z[i]) for i in bad[:FIRST]]))
    covc = _covered(lo[cont], hi[cont], z0, n)
    bad = np.nonzero(covc & ~inside)[0]
    if len(bad):
        out.append(("soundness", [int(z[i]) for i in bad[:FIRST]]))
    if exact:
        bad = np.nonzero(cov & ~inside)[0]
        if len(bad):
            out.append(("exact", [int(z[i]) for i in bad[:FIRST]]))
        bad = np.nonzero(~cont)[0]
        if len(bad):
            out.append(("not-contained", [(int(lo[i]), int(hi[i])) for i in bad[:FIRST]]))
    return out


# ---------------------------------------------------------------- XZ elements
def xz_elements(D, g):
    """Every element of levels 1..g of the XZ quad / oct tree over [0, 1]^D:
    (level [n], lower corner [n, D], width [n], code [n]).  An element is reached from the unit cell by
    child digits k_0 .. k_(level-1), bit d of k taking the upper half of dimension d (XElement.children,
    XZ2SFC.scala:406-415, XZ3SFC.scala:449-464); its code is sum_i 1 + k_i * (B^(g-i) - 1) / (B - 1),
    B = 2^D (sequenceCode, XZ2SFC.scala:264-286, XZ3SFC.scala:275-304).  Its enlarged cell is
    [corner, corner + 2 * width] per dimension."""
    B = 1 << D
    levels, corners, widths, codes = [], [], [], []
    for L in range(1, g + 1):
        side = 1 << L
        idx = np.arange(side ** D, dtype=np.int64)
        c = [(idx // (side ** d)) % side for d in range(D)]
        code = np.zeros(len(idx), np.int64)
        for i in range(L):
            k = np.zeros(len(idx), np.int64)
            for d in range(D):
                k |= ((c[d] >> (L - 1 - i)) & 1) << d
            code += 1 + k * ((B ** (g - i) - 1) // (B - 1))
        w = 2.0 ** -L
        levels.append(np.full(len(idx), L, np.int64))
        corners.append(np.stack([cd * w for cd in c], 1))
        widths.append(np.full(len(idx), w))
        codes.append(code)
    return np.concatenate(levels), np.concatenate(corners), np.concatenate(widths), np.concatenate(codes)


def xz_meets(corners, widths, windows, D):
    """Mask over elements: the enlarged cell meets some window (closed).  windows = [n, 2 * D] normalized,
    mins then maxs."""
    windows = np.asarray(windows, np.float64).reshape(-1, 2 * D)
    hit = np.zeros(len(widths), bool)
    for w in windows:
        ok = np.ones(len(widths), bool)
        for d in range(D):
            ok &= (w[D + d] >= corners[:, d]) & (w[d] <= corners[:, d] + 2.0 * widths)
        hit |= ok
    return hit


def in_ranges(lo, hi, v):
    """Mask over v: v lies in some range of an ascending, disjoint list."""
    v = np.asarray(v, np.int64)
    if len(lo) == 0:
        return np.zeros(v.shape, bool)
    order = np.argsort(lo, kind="stable")   # a broken list is not ascending: still a definite answer
    slo, shi = lo[order], np.maximum.accumulate(hi[order])
    k = np.searchsorted(slo, v, side="right") - 1
    return (k >= 0) & (v <= shi[np.maximum(k, 0)])


def check_xz_list(ranges, windows_normalized, D, g, elements=None):
    """An XZ2SFC.ranges / XZ3SFC.ranges list against every element of levels 1..g.  Only for windows
    whose normalized edges are not multiples of 2^-g, so that open against closed cannot matter.
      X1  Z1's ordering and merge rule, every lower >= 1                        "inverted" "order" "unmerged" "outside"
      X2  the code of every element whose enlarged cell meets a window is in a range         "cover"
      X3  every element whose code lies in a `contained` range meets a window               "soundness"
    """
    lo, hi, cont = as_arrays(ranges)
    _, corners, widths, codes = elements if elements is not None else xz_elements(D, g)
    out = []
    _order_violations(lo, hi, out)
    bad = np.nonzero(lo < 1)[0]
    if len(bad):
        out.append(("outside", [(int(lo[i]), int(hi[i])) for i in bad[:FIRST]]))
    meets = xz_meets(corners, widths, windows_normalized, D)
    bad = np.nonzero(meets & ~in_ranges(lo, hi, codes))[0]
    if len(bad):
        out.append(("cover", [int(codes[i]) for i in bad[:FIRST]]))
    bad = np.nonzero(in_ranges(lo[cont], hi[cont], codes) & ~meets)[0]
    if len(bad):
        out.append(("soundness", [int(codes[i]) for i in bad[:FIRST]]))
    return out


def check_cover(ranges, codes, hit, sound=None):
    """The end-to-end form, over indexed features:
      every feature with `hit` set has its code in a range                                   "cover"
      every feature whose code is in a `contained` range has `sound` set (default: `hit`)    "soundness"
    plus the ordering and merge rule ("inverted" "order" "unmerged").
    `sound` is for the Z curves, whose `contained` is decided on whole cells (ZN.scala:156-171 compares
    the cell's corners with the bounds' corners, themselves cells): a point of a boundary cell can lie
    outside the user-space box, so there `sound` is "the feature's cell lies inside some bound's cells"."""
    lo, hi, cont = as_arrays(ranges)
    codes = np.asarray(codes, np.int64)
    hit = np.asarray(hit, bool)
    sound = hit if sound is None else np.asarray(sound, bool)
    out = []
    _order_violations(lo, hi, out)
    bad = np.nonzero(hit & ~in_ranges(lo, hi, codes))[0]
    if len(bad):
        out.append(("cover", [(int(i), int(codes[i])) for i in bad[:FIRST]]))
    bad = np.nonzero(in_ranges(lo[cont], hi[cont], codes) & ~sound)[0]
    if len(bad):
        out.append(("soundness", [(int(i), int(codes[i])) for i in bad[:FIRST]]))
    return out


def kinds(violations):
    return sorted({k for k, _ in violations})
