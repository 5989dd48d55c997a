"""Python-integer models of the batched instance evaluation (spartan_amd/csrc/sparse_many.hip, sp_sparse_evaluate_many_begin): the sum it
computes for every (proof, matrix), and the half-table identity it replaces the full chi tables with. Test infrastructure only: no GPU, no
ctypes, no import of spartan_amd.

Every value is a RAW MONTGOMERY RESIDUE below q, as in tests/fq_reference.py, whose mm (the device's fq_mul) and chi_at are used here.
mm is commutative and associative and mm(x, ONE) = x, so a product of the same residues in any order and grouping is the same residue: the
device's hi_x lo_x hi_y lo_y val must come out as the model's chi(rx)[row] chi(ry)[col] val, limb for limb."""
import os, re
from tests import fq_reference as F
from tests.helpers import Q, RINV, ROOT

ONE, mm, chi_at = F.ONE, F.mm, F.chi_at
MAX_K = 64          # SP_EVAL_MANY_MAX_K
KS = (1, 2, 3, 5, 8, 33, 63, 64)                                   # every Kp in {1, 2, 4, 8, 64}, and K != Kp on both sides of a power of two
ELLS = ((1, 1), (1, 2), (2, 3), (3, 5), (8, 9), (13, 14))          # lo = 0, odd splits, non-square, both sides of EQ_SMALL_ELL = 13
NNZS = (0, 1, 255, 256, 257)


def split(ell):
    """(hi, lo) variables of the two half tables of an ell-variable point"""
    return ell - ell // 2, ell // 2


def half_tables(r):
    """(chi(r_hi), chi(r_lo)) in full: what k_eq_half_many builds per proof and side; the low half of a one-variable point is [ONE]"""
    hi, _ = split(len(r))
    return F.chi(r[:hi]), F.chi(r[hi:])


def chi_from_halves(r, i):
    """entry i of chi(r) by the identity chi(r)[i] = chi(r_hi)[i >> lo] chi(r_lo)[i & (2^lo - 1)]"""
    hi, lo = split(len(r))
    return mm(chi_at(r[:hi], i >> lo), chi_at(r[hi:], i & ((1 << lo) - 1)))


def evaluate_many(mats, rxs, rys):
    """out[k][m] = sum over the entries (row, col, val) of mats[m] of val chi(rxs[k])[row] chi(rys[k])[col]"""
    out = []
    for rx, ry in zip(rxs, rys):
        cx, cy = {}, {}
        vals = []
        for M in mats:
            acc = 0
            for row, col, val in M:
                if row not in cx:
                    cx[row] = chi_at(rx, row)
                if col not in cy:
                    cy[col] = chi_at(ry, col)
                acc += mm(mm(cx[row], cy[col]), val)
            vals.append(acc % Q)
        out.append(vals)
    return out


def dense_mle(M, rx, ry):
    """The multilinear extension of a dense 2^len(rx) x 2^len(ry) matrix of field VALUES (not residues) at the point (rx, ry), values too, by
    folding one variable at a time from the top (DensePolynomial::bound_poly_var_top): another algorithm than the sum over chi"""
    rows = [list(r) for r in M]
    for x in rx:
        h = len(rows) // 2
        rows = [[(a + x * (b - a)) % Q for a, b in zip(rows[i], rows[i + h])] for i in range(h)]
    v = rows[0]
    for y in ry:
        h = len(v) // 2
        v = [(v[j] + y * (v[j + h] - v[j])) % Q for j in range(h)]
    return v[0]


def partials_cap():
    """the cap of the partials grid, read from the source: a renamed or re-expressed constant raises"""
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", "sparse_many.hip")).read()
    m = re.search(r"\bEM_MAX_BLOCKS\s*=\s*(\d+)\b", src)
    if not m or "grid_for(max_nnz << lg_kp, EM_MAX_BLOCKS)" not in src:
        raise AssertionError("tests/eval_many_reference.py: sparse_many.hip no longer sizes its grid as grid_for(max_nnz << lg_kp, EM_MAX_BLOCKS)")
    return int(m.group(1))


def padded(K):
    kp = 1
    while kp < K:
        kp *= 2
    return kp


def blocks(max_nnz, K):
    """blocks per matrix of a call (grid_for over (entry, padded proof) lanes, 256 a block)"""
    return max(1, min(partials_cap(), (max(max_nnz, 1) * padded(K) + 255) // 256))


def nnz_at_cap(K):
    """the smallest nnz whose grid reaches the cap, and one that needs a second grid-stride pass of the first block"""
    per_block = 256 // padded(K)
    at = (partials_cap() - 1) * per_block + 1
    return at, partials_cap() * per_block + 1
