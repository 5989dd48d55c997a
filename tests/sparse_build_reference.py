"""Python-integer model of Instance::new (src/lib.rs:121-227): the padding rules, the per-entry checks in the reference's order, the column
shift, the pad entries and the four-word report of sp_sparse_from_entries — what the device build (spartan_amd/csrc/sparse_build.hip), the
host driver above it and the Python binding are compared with, exactly. Entries are (row, col, value) with plain integers: a row or a column
may be any 64-bit value, a value any 256-bit one. Also the products of a built matrix by big-int arithmetic, for the kernel-level tests."""
from tests.helpers import Q

NONE = 2**64 - 1                      # a report word of a class that is absent
OK, EINVAL, ESCALAR, EINDEX = 0, -1, -5, -6
BAD_SCALARS = [Q, Q + 1, 2**255, 2**256 - 1]


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def padded(num_cons, num_vars, num_inputs):
    """(num_cons_padded, num_vars_padded) of lib.rs:129-156, statement by statement: num_cons = 0 gives 1, not 2, because the second rule
    (0usize.next_power_of_two() = 1 != 0) overrides the first; tests/structured_cases.padded_shape agrees wherever num_cons >= 1"""
    nvp = next_pow2(max(num_vars, num_inputs + 1))
    ncp = num_cons
    if num_cons in (0, 1):
        ncp = 2
    if next_pow2(num_cons) != num_cons:
        ncp = next_pow2(num_cons)
    return ncp, nvp


def geometry(num_cons, num_vars, num_inputs, nnz):
    """the arguments sp_sparse_from_entries gets for a matrix of nnz entries of such an instance, as a dict"""
    ncp, nvp = padded(num_cons, num_vars, num_inputs)
    pad = ncp - nnz if num_cons in (0, 1) and nnz < ncp else 0          # lib.rs:191-195: for i in tups.len()..num_cons_padded
    return dict(row_limit=num_cons, col_limit=num_vars + 1 + num_inputs, col_split=num_vars, col_shift=nvp - num_vars, pad_count=pad,
                pad_col=num_vars, num_rows=ncp, num_cols=2 * nvp)


def invalid_arguments(nnz, g):
    """the SP_EINVAL conditions of the geometry (null pointers aside)"""
    total = nnz + g["pad_count"]
    return (g["num_rows"] == 0 or g["num_cols"] == 0 or g["num_rows"] >= 2**32 or g["num_cols"] >= 2**32 or total >= 2**32 - 1
            or g["row_limit"] > g["num_rows"] or g["col_limit"] + g["col_shift"] > g["num_cols"]
            or (g["pad_count"] and (total > g["num_rows"] or g["pad_col"] >= g["num_cols"])))


def build(entries, g):
    """(status, report, entries as stored or None). Every entry is classified, as the device does it: a bad index is counted whatever the
    value; a bad scalar only under a good index (lib.rs:164-186). The status is that of the lowest failing entry: where the loop returns."""
    rep = [0, NONE, 0, NONE]
    out = []
    for e, (r, c, v) in enumerate(entries):
        assert 0 <= r < 2**64 and 0 <= c < 2**64 and 0 <= v < 2**256
        if r >= g["row_limit"] or c >= g["col_limit"]:
            rep[0] += 1; rep[1] = min(rep[1], e)
        elif v >= Q:
            rep[2] += 1; rep[3] = min(rep[3], e)
        else:
            out.append((r, c + g["col_shift"] if c >= g["col_split"] else c, v))
    if rep[0] or rep[2]:
        return (EINDEX if rep[1] < rep[3] else ESCALAR), rep, None
    out += [(e, g["pad_col"], 0) for e in range(len(entries), len(entries) + g["pad_count"])]
    return OK, rep, out


def instance_new(num_cons, num_vars, num_inputs, A, B, C):
    """("ok", (ncp, nvp), [A', B', C']) or (error name, failing matrix, its report): all of A, then B, then C (lib.rs:200-213)"""
    mats = []
    for k, m in enumerate((A, B, C)):
        st, rep, out = build(m, geometry(num_cons, num_vars, num_inputs, len(m)))
        if st != OK:
            return {EINDEX: "InvalidIndex", ESCALAR: "InvalidScalar"}[st], k, rep
        mats.append(out)
    return "ok", padded(num_cons, num_vars, num_inputs), mats


# ---- a built matrix by big-int arithmetic (entries with the same (row, col) add up)

def csr_order(ent):
    """the entries sorted by row, entry order kept within a row (a stable sort); csc_order by column"""
    return sorted(ent, key=lambda e: e[0])


def csc_order(ent):
    return sorted(ent, key=lambda e: e[1])


def mulvec(ent, z, num_rows):
    out = [0] * num_rows
    for r, c, v in ent:
        out[r] += v * z[c]
    return [x % Q for x in out]


def eval_table(ent, rx, num_cols):
    out = [0] * num_cols
    for r, c, v in ent:
        out[c] += rx[r] * v
    return [x % Q for x in out]


def evaluate(ent, tx, ty):
    return sum(tx[r] * ty[c] % Q * v for r, c, v in ent) % Q


def violated_rows(A, B, C, z, num_rows):
    a, b, c = (mulvec(m, z, num_rows) for m in (A, B, C))
    return [r for r in range(num_rows) if a[r] * b[r] % Q != c[r]]
