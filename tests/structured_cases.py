"""Structured R1CS instances for the whole-proof parity tests (tests/test_structured_cases.py: the oracle on the CPU; tests/test_gpu_structured.py
and tests/switch_worker.py: the library against it): several entries per constraint, matrices of different sizes, columns read from many rows,
a num_vars that is no power of two and a matrix without entries — the shapes produce_synthetic_r1cs never has. Plain Python, no GPU.

A case is a seeded function returning (num_cons, num_vars, num_inputs, A, B, C, vars, inputs). Entries are (row, col, int) in the CALLER's
column numbering of Instance::new (lib.rs:121-128): variables 0..num_vars, the constant at num_vars, the inputs after it. Every case is
satisfiable by construction (A, B and the assignment are chosen, then each row is solved for a term of C) and asserts what it claims to
reach by integer predicate before it returns, in the way of tests/field_vectors.py."""
import ctypes, hashlib, random
from tests.helpers import Q, mont_bulk, sz, vp, u64x4


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def _skewed_instance(rng, num_cons, num_vars, num_inputs, n_short, pool):
    """Row 0: A = every variable with a random coefficient (one (row, col) pair twice), B = the constant 1, C = the variable t = num_vars - 1,
    which the assignment sets to A's sum. Rows 1..n_short: 1-3 entries per matrix over the variables of `pool`, C's constant term chosen so
    that the row holds; one of them repeats a (row, col) pair in A. All other rows are empty. Returns entries (A, B, C) and the assignment."""
    t, const = num_vars - 1, num_vars
    v = [rng.randrange(Q) for _ in range(num_vars)]
    inputs = [rng.randrange(Q) for _ in range(num_inputs)]
    coef = [rng.randrange(1, Q) for _ in range(num_vars)]
    dup_col, dup_coef = 5, rng.randrange(1, Q)
    while coef[t] == 1:
        coef[t] = rng.randrange(2, Q)
    A = [(0, j, coef[j]) for j in range(num_vars)] + [(0, dup_col, dup_coef)]
    rng.shuffle(A)                                            # the long row's entries arrive in no particular order
    rest = (sum(coef[j] * v[j] for j in range(num_vars) if j != t) + dup_coef * v[dup_col]) % Q
    v[t] = rest * pow((1 - coef[t]) % Q, Q - 2, Q) % Q        # t = rest + coef[t] * t
    B, C = [(0, const, 1)], [(0, t, 1)]
    touching = {}
    for r in range(1, n_short + 1):
        ea = [(r, rng.choice(pool), rng.randrange(1, Q)) for _ in range(rng.randint(1, 3))]
        if r == 7:
            ea.append((r, ea[0][1], rng.randrange(1, Q)))     # the same (row, col) again: the two entries add up
        eb = [(r, rng.choice(pool + [const, const + 1]), rng.randrange(1, Q)) for _ in range(rng.randint(1, 2))]
        ec = [(r, rng.choice(pool), rng.randrange(1, Q)) for _ in range(rng.randint(0, 2))]
        zz = lambda c: v[c] if c < num_vars else ([1] + inputs)[c - num_vars]
        a = sum(x * zz(c) for _, c, x in ea) % Q
        b = sum(x * zz(c) for _, c, x in eb) % Q
        ec.append((r, const, (a * b - sum(x * zz(c) for _, c, x in ec)) % Q))
        A += ea; B += eb; C += ec
        for _, c, _x in ea + eb + ec:
            touching.setdefault(c, set()).add(r)
    return (A, B, C), v, inputs, touching


# ---- integer ground truth over a case

def failing_rows(case, vars_=None, inputs=None):
    """{r : (A z)[r] * (B z)[r] != (C z)[r]} by big-int arithmetic over z = (vars, 1, inputs) in the caller's numbering; every entry adds"""
    num_cons, num_vars, num_inputs, A, B, C, v, i = case
    z = list(v if vars_ is None else vars_) + [1] + list(i if inputs is None else inputs)
    assert len(z) == num_vars + 1 + num_inputs
    acc = []
    for m in (A, B, C):
        s = [0] * num_cons
        for r, c, x in m:
            s[r] += x * z[c]
        acc.append(s)
    return [r for r in range(num_cons) if (acc[0][r] % Q) * (acc[1][r] % Q) % Q != acc[2][r] % Q]


def padded_shape(case):
    """(num_cons_padded, num_vars_padded, column shift) of Instance::new (lib.rs:129-156, 178-182)"""
    num_cons, num_vars, num_inputs = case[:3]
    nvp = next_pow2(max(num_vars, num_inputs + 1))
    ncp = 2 if num_cons in (0, 1) else next_pow2(num_cons)
    return ncp, nvp, nvp - num_vars


def dense_stats(case):
    """What SNARK::encode makes of the case, restated from sparse_mlpoly.rs:221-254, 356-427 with Python lists: every matrix padded to
    N = max next_pow2(nnz) with (0, 0, 0) entries, cells = max(num_cons_padded, 2 num_vars_padded), one audit counter per cell running over
    A, B, C in turn. Returns N, cells, the largest read timestamp and the largest audit timestamp of the row and the column memory, the
    longest row and the largest number of distinct rows that touch one column."""
    num_cons, num_vars, num_inputs, A, B, C = case[:6]
    ncp, nvp, shift = padded_shape(case)
    N = max(next_pow2(len(m)) for m in (A, B, C))
    cells = max(ncp, 2 * nvp)
    out = {"N": N, "cells": cells, "nnz": [len(A), len(B), len(C)]}
    for side, pick in (("row", lambda e: e[0]), ("col", lambda e: e[1] + shift if e[1] >= num_vars else e[1])):
        audit = [0] * cells
        top = 0
        for m in (A, B, C):
            for a in [pick(e) for e in m] + [0] * (N - len(m)):
                top = max(top, audit[a])
                audit[a] += 1
        out["max_read_ts_" + side] = top
        out["max_audit_ts_" + side] = max(audit)
        out["hottest_cell_" + side] = audit.index(max(audit))
    per_row, per_col = {}, {}
    for k, m in enumerate((A, B, C)):
        for r, c, _ in m:
            per_row[(k, r)] = per_row.get((k, r), 0) + 1
            per_col.setdefault(c, set()).add(r)
    out["longest_row"] = max(per_row.values())
    out["rows_on_hottest_column"] = max(len(s) for s in per_col.values())
    out["empty_rows"] = sum(1 for r in range(num_cons) if all((k, r) not in per_row for k in range(3)))
    return out


def _duplicates(m):
    return len(m) - len(set((r, c) for r, c, _ in m))


def _zz(v, inputs, num_vars):
    return lambda c: v[c] if c < num_vars else ([1] + inputs)[c - num_vars]


def _close_rows(A, B, C, v, inputs, num_cons, num_vars, rows=None):
    """adds a constant term to C in every row (or in `rows`), chosen so that the row holds"""
    zz = _zz(v, inputs, num_vars)
    s = [[0] * num_cons for _ in range(3)]
    for k, m in enumerate((A, B, C)):
        for r, c, x in m:
            s[k][r] += x * zz(c)
    for r in (range(num_cons) if rows is None else rows):
        C.append((r, num_vars, (s[0][r] * s[1][r] - s[2][r]) % Q))


def _checked(name, case, N, cells):
    st = dense_stats(case)
    assert failing_rows(case) == [], name                      # every row holds in big-int arithmetic
    assert (st["N"], st["cells"]) == (N, cells), (name, st)
    w = list(case[6]); j = BREAKING_VAR[name]
    w[j] = (w[j] + 1) % Q
    assert failing_rows(case, vars_=w), name                   # and one changed variable breaks at least one
    return st


BREAKING_VAR = {"ops_heavy": 63, "long_row_hot_column": 3, "shifted": 99, "c_sparse": 2, "c_empty": 2, "ops_heavy_17": 2047}


def ops_heavy():
    """64 / 64 / 5. A: 33 entries in every row (nnz = 2112, a little above 2^11: N = 4096). B: 4-5 entries per row. C: a constant term per
    row and six more. cells = 128, so num_ops = 32 cells; B and C are padded with thousands of (0, 0, 0) entries, all of them reads of cell 0."""
    rng = random.Random(0x0905)
    nc, nv, ni = 64, 64, 5
    ncols = nv + 1 + ni
    v = [rng.randrange(Q) for _ in range(nv)]; inputs = [rng.randrange(Q) for _ in range(ni)]
    A = [(r, c, rng.randrange(1, Q)) for r in range(nc) for c in rng.sample(range(ncols), 33)]
    B = [(r, c, rng.randrange(1, Q)) for r in range(nc) for c in rng.sample(range(ncols), rng.randint(4, 5))]
    C = [(rng.randrange(nc), rng.randrange(nv), rng.randrange(1, Q)) for _ in range(6)]
    _close_rows(A, B, C, v, inputs, nc, nv)
    rng.shuffle(A)                                            # entries of one row are not adjacent in M
    case = (nc, nv, ni, A, B, C, v, inputs)
    st = _checked("ops_heavy", case, 4096, 128)
    assert len(A) == 2112 and 256 < len(B) <= 320 and len(C) == 70 and st["N"] == 32 * st["cells"]
    assert next_pow2(len(B)) == 512 and next_pow2(len(C)) == 128
    pads = 2 * st["N"] - len(B) - len(C)                      # (0, 0, 0) entries: each one reads cell 0 of both memories
    assert pads > 7000 and st["hottest_cell_row"] == 0 and st["hottest_cell_col"] == 0
    assert st["max_read_ts_row"] >= pads and st["max_read_ts_col"] >= pads and st["max_audit_ts_row"] == st["max_read_ts_row"] + 1
    assert st["longest_row"] == 33 and st["empty_rows"] == 0
    return case


def long_row_hot_column():
    """256 / 1024 / 2: _skewed_instance scaled down. Row 0 of A reads every variable (1025 entries, one pair twice), 60 short rows over a pool of
    16 variables, B reads the constant and an input from several rows, the constant column of C is read by every short row; rows 61..255 are
    empty. N = cells = 2048."""
    rng = random.Random(0x10c0)
    nc, nv, ni, n_short = 256, 1024, 2, 60
    (A, B, C), v, inputs, touching = _skewed_instance(rng, nc, nv, ni, n_short, list(range(16)))
    # on top of it B reads the constant from every second short row and the first input from every third; C's constant terms are solved again
    B += [(r, nv, rng.randrange(1, Q)) for r in range(2, n_short + 1, 2)] + [(r, nv + 1, rng.randrange(1, Q)) for r in range(3, n_short + 1, 3)]
    C[:] = [e for e in C if e[1] != nv]
    _close_rows(A, B, C, v, inputs, nc, nv, rows=range(1, n_short + 1))
    case = (nc, nv, ni, A, B, C, v, inputs)
    st = _checked("long_row_hot_column", case, 2048, 2048)
    assert st["longest_row"] == 1025 and sum(1 for r, _, _ in A if r == 0) == 1025
    pairs = [(r, c) for r, c, _ in A]
    assert pairs.count((0, 5)) == 2 and any(pairs.count(p) >= 2 for p in pairs if p[0] == 7)   # the two stated duplicates
    assert _duplicates(A) >= 2                                # choosing from a pool of 16 repeats a few more pairs in the short rows
    assert st["empty_rows"] == nc - 1 - n_short
    assert len(touching[nv]) == n_short and st["rows_on_hottest_column"] == n_short + 1   # the constant column: row 0 and every short row
    assert len({r for r, c, _ in B if c == nv}) >= 30 and len({r for r, c, _ in B if c == nv + 1}) >= 20
    assert max(len(touching[j]) for j in range(16)) >= 12     # and pool variables by a dozen and more
    return case


def shifted():
    """37 / 100 / 7: 2-4 entries per row and matrix over the variables, the constant and every input; four entries whose value is explicitly 0;
    the last row and the last variable are used. Instance::new pads to 64 / 128 and moves the constant and the inputs up by 28."""
    rng = random.Random(0x5f1d)
    nc, nv, ni = 37, 100, 7
    ncols = nv + 1 + ni
    v = [rng.randrange(1, Q) for _ in range(nv)]; inputs = [rng.randrange(1, Q) for _ in range(ni)]
    A, B, C = [], [], []
    for r in range(nc):
        ca = rng.sample(range(ncols), rng.randint(2, 4))
        if r < ni + 1 and nv + r not in ca:
            ca[0] = nv + r                                    # the constant and each input, in A
        cb = rng.sample(range(ncols), rng.randint(2, 4))
        if r >= nc - (ni + 1) and nv + (nc - 1 - r) not in cb:
            cb[0] = nv + (nc - 1 - r)                         # and again in B, from the last rows
        if r == nc - 1 and nv - 1 not in cb:
            cb[1] = nv - 1                                    # the last variable in the last row
        cc = rng.sample([c for c in range(ncols) if c != nv], rng.randint(1, 3))
        A += [(r, c, rng.randrange(1, Q)) for c in ca]
        B += [(r, c, rng.randrange(1, Q)) for c in cb]
        C += [(r, c, rng.randrange(1, Q)) for c in cc]
    zero_at = {0: (3, 1), 1: (10, 0), 2: (20, 0)}             # matrix -> (row, which entry of the row) gets the value 0
    for k, m in enumerate((A, B, C)):
        row, which = zero_at[k]
        idx = [i for i, e in enumerate(m) if e[0] == row][which]
        m[idx] = (m[idx][0], m[idx][1], 0)
    A.append((5, 17, 0))                                      # a zero entry on a (row, col) of its own
    _close_rows(A, B, C, v, inputs, nc, nv)
    case = (nc, nv, ni, A, B, C, v, inputs)
    st = _checked("shifted", case, 128, 256)
    assert padded_shape(case) == (64, 128, 28)
    per = lambda m, r: sum(1 for e in m if e[0] == r)
    assert all(2 <= per(m, r) <= 4 for m in (A, B, C) for r in range(nc) if (m, r) != (A, 5)) and 2 <= per(A, 5) <= 5
    for m in (A, B):
        assert {c for _, c, _ in m} >= set(range(nv, ncols))  # the constant and every input
    assert sum(1 for m in (A, B, C) for e in m if e[2] == 0) == 4 and all(x != 0 for r, c, x in C if c == nv)
    assert any(e[0] == nc - 1 and e[1] == nv - 1 for e in B)
    return case


def _selector_case(name, seed, c_rows):
    """32 / 32 / 1 with one entry per row in A and in B. In the rows of c_rows A selects a non-zero variable and C holds one entry that makes
    the row hold; in every other row A selects a variable whose value is 0 and C has nothing: 0 * b = 0."""
    rng = random.Random(seed)
    nc, nv, ni = 32, 32, 1
    v = [0 if j < 4 else rng.randrange(1, Q) for j in range(nv)]
    inputs = [rng.randrange(1, Q)]
    zz = _zz(v, inputs, nv)
    A, B, C = [], [], []
    for r in range(nc):
        a = (r, rng.randrange(4, nv) if r in c_rows else rng.randrange(4), rng.randrange(1, Q))
        b = (r, rng.randrange(4, nv + 2), rng.randrange(1, Q))
        A.append(a); B.append(b)
        if r in c_rows:
            j = rng.randrange(4, nv)
            C.append((r, j, a[2] * zz(a[1]) * b[2] * zz(b[1]) * pow(v[j], Q - 2, Q) % Q))
    case = (nc, nv, ni, A, B, C, v, inputs)
    st = _checked(name, case, 32, 64)
    assert st["nnz"] == [32, 32, len(c_rows)] and {r for r, _, _ in C} == set(c_rows)
    assert all(v[c] == 0 for r, c, _ in A if r not in c_rows) and all(zz(c) != 0 for _, c, _ in B)
    assert st["max_read_ts_row"] >= 32 - len(c_rows)          # C's padding reads cell 0
    return case


def c_sparse():
    """32 / 32 / 1, nnz = 32 / 32 / 3: C is almost entirely padding, 29 rows are 0 = 0."""
    return _selector_case("c_sparse", 0xc5, (5, 17, 31))


def c_empty():
    """32 / 32 / 1, nnz = 32 / 32 / 0: a matrix with no entry at all (the reference accepts it: an empty M, num_nz_entries =
    0usize.next_power_of_two() = 1, all of C's dense vectors are padding)."""
    case = _selector_case("c_empty", 0xce, ())
    assert case[5] == []
    return case


def ops_heavy_17():
    """2^11 / 2^11 / 10. A: 64 entries per row (nnz = N = 2^17). B: 4 per row (2^13). C: a variable and a constant term per row (2^12).
    cells = 2^12: the throughput-sized batched rounds at num_ops = 32 cells."""
    rng = random.Random(0x17)
    nc = nv = 1 << 11
    ni = 10
    ncols = nv + 1 + ni
    rnd = lambda: rng.getrandbits(300) % (Q - 1) + 1
    v = [rnd() for _ in range(nv)]; inputs = [rnd() for _ in range(ni)]
    A = [(r, c, rnd()) for r in range(nc) for c in rng.sample(range(ncols), 64)]
    B = [(r, c, rnd()) for r in range(nc) for c in rng.sample(range(ncols), 4)]
    C = [(r, rng.randrange(nv), rnd()) for r in range(nc)]
    C[-1] = (nc - 1, nv - 1, C[-1][2])                        # the last variable is read, and decides the last row
    _close_rows(A, B, C, v, inputs, nc, nv)
    case = (nc, nv, ni, A, B, C, v, inputs)
    st = _checked("ops_heavy_17", case, 1 << 17, 1 << 12)
    assert st["nnz"] == [1 << 17, 1 << 13, 1 << 12] and st["N"] == 32 * st["cells"] and st["longest_row"] == 64
    assert st["max_read_ts_row"] >= 2 * (1 << 17) - (1 << 13) - (1 << 12)
    return case


SMALL = {"ops_heavy": ops_heavy, "long_row_hot_column": long_row_hot_column, "shifted": shifted, "c_sparse": c_sparse, "c_empty": c_empty}
CASES = dict(SMALL, ops_heavy_17=ops_heavy_17)
# the RandomTape seed of each case, pinned by name (the committed digests depend on it); labels are the examples' (b"snark_example", b"nizk_example")
TAPE_SEED = {"ops_heavy": 500, "long_row_hot_column": 501, "shifted": 502, "c_sparse": 503, "c_empty": 504, "ops_heavy_17": 505}
assert set(TAPE_SEED) == set(CASES) == set(BREAKING_VAR)
SNARK_LABEL, NIZK_LABEL = b"snark_example", b"nizk_example"
_cache = {}


def get(name):
    """the case, built once per process (the tests share it and leave it unchanged)"""
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


# ---- the case as the C entry points take it (product and oracle alike)

class Packed:
    """nnz[3], rows / cols (uint64, A, B, C back to back), vals (32 canonical little-endian bytes each), the assignment as Montgomery limbs:
    vars as the caller holds them (num_vars of them) and zero-padded to num_vars_padded (what the oracle's handle keeps), inputs"""
    def __init__(self, case, vars_=None, inputs=None):
        num_cons, num_vars, num_inputs, A, B, C, v, i = case
        v = list(v if vars_ is None else vars_); i = list(i if inputs is None else inputs)
        ent = A + B + C
        self.num_cons, self.num_vars, self.num_inputs = num_cons, num_vars, num_inputs
        self.nnz = [len(A), len(B), len(C)]
        self.rows = (ctypes.c_uint64 * len(ent))(*[e[0] for e in ent])
        self.cols = (ctypes.c_uint64 * len(ent))(*[e[1] for e in ent])
        self.vals = b"".join(e[2].to_bytes(32, "little") for e in ent)
        self.nvp = padded_shape(case)[1]
        self.vars = mont_bulk(v)
        self.vars_padded = mont_bulk(v + [0] * (self.nvp - num_vars))
        self.inputs = mont_bulk(i)

    def oracle_instance(self, orc):
        err = ctypes.c_int(0)
        oi = vp(orc.orc_instance_new_padded(sz(self.num_cons), sz(self.num_vars), sz(self.num_inputs), (sz * 3)(*self.nnz), self.rows, self.cols,
                                            self.vals, self.vars_padded, sz(self.nvp), self.inputs, ctypes.byref(err)))
        assert err.value == 0 and oi
        return oi


def oracle_bytes(orc, fn, h):
    n = fn(h, None, sz(0)); b = (ctypes.c_uint8 * n)(); fn(h, b, sz(n))
    return bytes(b)


class OracleRun:
    """The oracle's side of one case: instance, generators, SNARK::encode, SNARK::prove and NIZK::prove (set_digest(b"<case name>")) with the
    case's tape, kept as handles and bytes. Every consumer reads it; none changes it."""
    def __init__(self, orc, name):
        self.name, self.case = name, get(name)
        self.pk = pk = Packed(self.case)
        self.digest = name.encode()
        self.tape = u64x4(); orc.orc_seed_scalar(b"tape", ctypes.c_uint64(TAPE_SEED[name]), self.tape)
        self.oi = pk.oracle_instance(orc)
        self.gens_args = (pk.num_cons, pk.num_vars, pk.num_inputs, max(pk.nnz))
        self.og = vp(orc.orc_snark_gens_new(*[sz(x) for x in self.gens_args]))
        self.ong = vp(orc.orc_nizk_gens_new(*[sz(x) for x in self.gens_args[:3]]))
        self.oe = vp(orc.orc_snark_encode(self.oi, self.og))
        self.commitment = oracle_bytes(orc, orc.orc_commitment_bincode, self.oe)
        self.op = vp(orc.orc_snark_prove(self.oi, self.og, self.oe, SNARK_LABEL, self.tape, None))
        self.snark = oracle_bytes(orc, orc.orc_proof_bytes, self.op)
        self.onp = vp(orc.orc_nizk_prove(self.oi, self.ong, self.digest, sz(len(self.digest)), NIZK_LABEL, self.tape, None))
        self.nizk = oracle_bytes(orc, orc.orc_proof_bytes, self.onp)
        lens = (ctypes.c_size_t * 3)()
        orc.orc_proof_part_lens(self.op, lens)
        self.snark_sat_len = int(lens[0])

    def wrong_inputs(self):
        """the inputs with the first one changed (Montgomery limbs): what the verifiers must reject the proofs against"""
        i = list(self.case[7]); i[0] = (i[0] + 1) % Q
        return mont_bulk(i)

    def wrong_inputs_instance(self):
        """the same instance with those inputs"""
        i = list(self.case[7]); i[0] = (i[0] + 1) % Q
        return Packed(self.case, inputs=i)

    def entry(self):
        """what tests/golden/proof_digests.json keeps of the case"""
        sha = lambda b: hashlib.sha256(b).hexdigest()
        l0 = self.snark_sat_len
        return {"snark": {"len": len(self.snark), "sha256": sha(self.snark), "sat_len": l0, "sat_sha256": sha(self.snark[:l0]),
                          "rest_sha256": sha(self.snark[l0:])},
                "nizk": {"len": len(self.nizk), "sha256": sha(self.nizk)},
                "commitment": {"len": len(self.commitment), "sha256": sha(self.commitment)}}

    def free(self, orc):
        orc.orc_proof_free(self.op); orc.orc_proof_free(self.onp); orc.orc_encode_free(self.oe)
        orc.orc_snark_gens_free(self.og); orc.orc_nizk_gens_free(self.ong); orc.orc_instance_free(self.oi)


_runs = {}


def oracle_run(orc, name):
    """the OracleRun of a case, computed once per process and shared (tests/golden/make_golden.py and the tests read the same one)"""
    if name not in _runs:
        _runs[name] = OracleRun(orc, name)
    return _runs[name]
