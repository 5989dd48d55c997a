"""Python-integer models of the SPARK kernel family (spartan_amd/csrc/spark.hip: the batched cubic sum-check, the product trees, the hash
layers, dot_many / dot3) and a restatement of its host-side dispatch arithmetic. Test infrastructure only: no GPU, no ctypes, no import
of spartan_amd.

Every value is a RAW MONTGOMERY RESIDUE below q, as in tests/field_vectors.py and the `_table` / `mm` of tests/test_gpu_field_lanes.py: the
device's fq_mul is mm(a, b) = a b R^-1 mod q, its fq_add / fq_sub are plain addition and subtraction mod q, and the residue of one is
R mod q. Tables come straight from the Fq edge pool (the operands of every class of field_vectors.layout_a("fq")), so the 32-bit word
patterns that steer the device's carry chains reach the kernels unchanged.

The models are written from the formulas in the comments of spark.hip (and the lines of sumcheck.rs / product_tree.rs / sparse_mlpoly.rs
those cite). Sums are accumulated as exact integers and reduced once: mm(mm(a, b), c) = a b c R^-2 mod q.

plan(...) restates which kernel form and which summation path a call takes. Its only purpose is to keep the case lists of
tests/test_gpu_spark_edges.py on the boundaries of the dispatch (tests/test_spark_reference.py checks that); it is never an expected value
for device output."""
import os, random, re
from tests import field_vectors as V
from tests.helpers import Q, R, RINV, ROOT

ONE = R % Q                 # the residue of 1
RINV2 = RINV * RINV % Q
HALF = pow(2, Q - 2, Q) * R % Q   # the residue of 1/2
_POOL = []


def mm(a, b):
    return a * b * RINV % Q     # Montgomery product of residues


def edge_pool():
    if not _POOL:
        _POOL.extend(x for _, a, b in V.layout_a("fq") for x in (a, b))
    return _POOL


def edge_table(layout, n, k):
    """n residues from the edge pool: (a) neighbours differ, (c) runs of 64 equal values (a whole wavefront carries the same way); k: which
    table of a set. The indexing of test_gpu_field_lanes._table."""
    pool = edge_pool()
    off = 977 * k % len(pool)
    rot = pool[off:] + pool[:off]
    if layout == "a":      # entry i = pool[(off + i) % len(pool)]
        return (rot * (n // len(rot) + 1))[:n]
    runs = (rot * (n // (64 * len(rot)) + 1))[:(n + 63) // 64]      # entry i = pool[(off + i // 64) % len(pool)]
    return [x for x in runs for _ in range(64)][:n]


def nonzero_edge_table(layout, n, k):
    """edge_table with q - 1 in the place of zero: leaves of a product tree (one zero leaf makes every layer above it zero)"""
    return [x if x else Q - 1 for x in edge_table(layout, n, k)]


def edge_challenges(seed):
    """the cycle of challenges and weights: the residues 0, R mod q (one), q - 1 and a seeded random one"""
    return [0, ONE, Q - 1, random.Random(seed).randrange(Q)]


# ------------------------------------------------------------------ the cubic sum-check
def _halves(T):
    h = len(T) // 2
    return T[:h], T[h:]


def _lines(T):
    """the lines through (0, T[i]), (1, T[i + len/2]) at t = 0, 1, 2, 3 (integers, not reduced)"""
    x0, x1 = _halves(T)
    x2 = [2 * v - u for u, v in zip(x0, x1)]
    return x0, x1, x2, [w + v - u for u, v, w in zip(x0, x1, x2)]


def _sum3(a, b, c):
    return sum(x * y * z for x, y, z in zip(a, b, c)) * RINV2 % Q


def cubic_evals4(A, B, C):
    """sum_i A(t) B(t) C(t) at t = 0, 1, 2, 3 over the top-variable pairs (i, i + len/2) (sumcheck.rs:290-357; cubic_point<4>)"""
    return [_sum3(a, b, c) for a, b, c in zip(_lines(A), _lines(B), _lines(C))]


def cubic_evals(A, B, C):
    """... at t = 0, 2, 3 (cubic_point)"""
    la, lb, lc = _lines(A), _lines(B), _lines(C)
    return [_sum3(la[t], lb[t], lc[t]) for t in (0, 2, 3)]


def bind(T, r):
    """bound_poly_var_top: T'[i] = T[i] + r (T[i + len/2] - T[i])"""
    x0, x1 = _halves(T)
    rc = r * RINV % Q
    return [(u + rc * (v - u)) % Q for u, v in zip(x0, x1)]


def quad_eq(A, B, Ceq):
    """q(0), q(2) of quad_point_eq: q(t) = sum_x A(t, x) B(t, x) Ceq[x] over the LEADING len/2 entries of the unbound eq table"""
    la, lb = _lines(A), _lines(B)
    return [_sum3(la[0], lb[0], Ceq), _sum3(la[2], lb[2], Ceq)]


def quad_eq_at(A, B, Ceq, t):
    """q(t) at any small integer t (the host derives q(1) and q(3); here for the identity kappa(t) q(t) = E(t))"""
    h = len(A) // 2
    return sum((A[i] + t * (A[h + i] - A[i])) * (B[i] + t * (B[h + i] - B[i])) * Ceq[i] for i in range(h)) * RINV2 % Q


def eq_table(rho):
    """EqPolynomial::new(rho).evals() on residues: entry x = prod_k eq(x_k, rho_k), rho[0] the top variable"""
    chi = [ONE]
    for rj in rho:
        chi = [x for e in chi for x in (mm(e, (ONE - rj) % Q), mm(e, rj))]
    return chi


def eq_at(t, rho):
    """eq(t, rho) = (1 - t)(1 - rho) + t rho at an INTEGER t (0..3); rho and the result are residues"""
    return ((1 - t) * (ONE - rho) + t * rho) % Q


def bind2_coeffs(A, B, C):
    """The twelve values (M0, M3, T1, T2) x t in {0, 2, 3} of the comment above k_cubic_bind2_eval: with x0..x3 the entries (i, i + q, i + 2q,
    i + 3q) of a table of length 4q, P(t) the line through (x0, x1) and U(t) the line through (x2, x3):
    M0 = sum P_A P_B P_C, M3 = sum U_A U_B U_C, T1 = sum (P+U)(P+U)(P+U), T2 = sum (P-U)(P-U)(P-U). Order: [4 t' + {0, 1, 2, 3}]."""
    q = len(A) // 4
    out = []
    for t in (0, 2, 3):
        m0 = m3 = t1 = t2 = 0
        for i in range(q):
            P = [T[i] + t * (T[i + q] - T[i]) for T in (A, B, C)]
            U = [T[i + 2 * q] + t * (T[i + 3 * q] - T[i + 2 * q]) for T in (A, B, C)]
            m0 += P[0] * P[1] * P[2]
            m3 += U[0] * U[1] * U[2]
            t1 += (P[0] + U[0]) * (P[1] + U[1]) * (P[2] + U[2])
            t2 += (P[0] - U[0]) * (P[1] - U[1]) * (P[2] - U[2])
        out += [m0 * RINV2 % Q, m3 * RINV2 % Q, t1 * RINV2 % Q, t2 * RINV2 % Q]
    return out


def predict(coeffs, r):
    """the evaluations at t = 0, 2, 3 of the round AFTER a bind at r, from (M0, M3, T1, T2) per t, as the host driver evaluates the cubic:
    M1 = (T1 - T2)/2 - M3, M2 = (T1 + T2)/2 - M0, E = (1-r)^3 M0 + (1-r)^2 r M1 + (1-r) r^2 M2 + r^3 M3"""
    om = (ONE - r) % Q
    om2, r2 = mm(om, om), mm(r, r)
    out = []
    for k in range(len(coeffs) // 4):
        M0, M3, T1, T2 = coeffs[4 * k:4 * k + 4]
        M1 = (mm((T1 - T2) % Q, HALF) - M3) % Q
        M2 = (mm((T1 + T2) % Q, HALF) - M0) % Q
        out.append((mm(mm(om2, om), M0) + mm(mm(om2, r), M1) + mm(mm(om, r2), M2) + mm(mm(r2, r), M3)) % Q)
    return out


def weighted(per_instance, w):
    """sum_k w_k v_k[j] for every component j (the `coeffs` of sumcheck.rs:359-369 applied per instance, instances added up)"""
    return [sum(wk * v[j] for wk, v in zip(w, per_instance)) * RINV % Q for j in range(len(per_instance[0]))]


# ------------------------------------------------------------------ hash layers, product trees, reductions
def hash_leaf(addr, val, ts, inc, rh, rm):
    """(ts + inc) r_hash^2 + val r_hash + addr - r_multiset (sparse_mlpoly.rs:529-604); inc is 0 or 1, everything else a residue"""
    return (mm((ts + inc * ONE) % Q, mm(rh, rh)) + mm(val, rh) + addr - rm) % Q


def index_residue(i):
    """fq_from_u64(i): the residue of the integer i"""
    return i * R % Q


def product_layers(leaves):
    """ProductCircuit::new (product_tree.rs:36-56): layer k+1 [i] = layer k [i] * layer k [i + len/2], down to the two roots; returned in the
    store's layout, layer k+1 behind layer k: 2 n - 2 entries"""
    store, cur = list(leaves), list(leaves)
    while len(cur) > 2:
        h = len(cur) // 2
        cur = [mm(cur[i], cur[h + i]) for i in range(h)]
        store += cur
    return store


def dot_many(chi, tabs):
    n = len(chi)
    return [sum(chi[i] * t[i] for i in range(n)) * RINV % Q for t in tabs]


def dot3(l, r, w):
    return sum(a * b * c for a, b, c in zip(l, r, w)) * RINV2 % Q


# ------------------------------------------------------------------ the dispatch arithmetic, restated
def _constant(path, name):
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", path)).read()
    m = re.search(r"\b%s\s*=\s*(\d+)\b" % name, src)
    if not m:
        raise AssertionError("tests/spark_reference.py: the constant %s is no longer defined as a literal in spartan_amd/csrc/%s: "
                             "restate plan() against the new source" % (name, path))
    return int(m.group(1))


_CONST = {}


def constants():
    if not _CONST:
        _CONST.update(HOST_SUM_BYTES=_constant("internal.hpp", "HOST_SUM_BYTES"), TAIL_OFF=_constant("spark.hip", "TAIL_OFF"),
                      TAIL_MAX_INST=_constant("spark.hip", "TAIL_MAX_INST"))
    return _CONST


def _grid_for(work, maxblocks=2048):
    return max(1, min(maxblocks, (work + 255) // 256))     # internal.hpp, grid_for


TINY_MAX = 8192          # spark.hip, batched_plan: `p->work <= 8192`, work = half (eval) or quarter (bind_eval)
INLINE_MAX_INST = 24     # spark.hip, place_triples: `inline_args && ninst <= 24`, for the one-round and the two-round calls; struct TripleInline / Bind2Inline
TREE_TAIL_MAX = 2048     # spark.hip, sp_product_tree_many_from: `if (len <= 2048)`: the remaining layers in one launch
TREE_TWO_MIN = 8192      # spark.hip, sp_product_tree_many_from: `len <= l2max && len >= 8192`: two layers per launch
TREE_TWO_MAX_LOG2 = 18   # options.hpp:50 spark.prod_layer2_max_log2, default 18
TREE_CHUNK = 16          # spark.hip, sp_product_tree_many_from: `for (k0 = 0; k0 < count; k0 += 16)`, struct Stores16
EQ_MIN_LEN = 65536       # spark.hip, batched_round: `len < (eq ? 65536 : ..)`
EQ_MAX_INST = 24         # spark.hip, eq_form_check: `ninst > 24`
MAX_INST = 64            # spark.hip, batched_round and bind2_launch: `ninst > 64`
# the dispatch of a batched round is decided in ONE place each (batched_plan, place_triples, build_triples, sum_partials_on_host): the tiny
# threshold, the inline-arguments test, the first-user-of-a-distinct-C scan and the host-side sum of the per-block partials. A second copy of
# one of them could drift unnoticed (tests/test_spark_reference.py counts them)
SOURCE_TEXT_ONCE = [
    "p->tiny = !eq && p->work <= 8192;",
    "inline_args && ninst <= 24",
    "first = first && C[m] != C[k];",
    "acc = fq_add(acc, p[(i * nblk + b) * K + k]);",
]
SOURCE_FRAGMENT_ONCE = ["tiny = ", "ninst <= 24", "first && C[", "nblk + b) *"]


def source_text_counts():
    """how often spark.hip contains each entry of SOURCE_TEXT_ONCE and its distinctive fragment (a copy under other variable names)"""
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", "spark.hip")).read()
    return {t: src.count(t) for t in SOURCE_TEXT_ONCE + SOURCE_FRAGMENT_ONCE}


def plan(call, length=0, ninst=1, nbind=0, want_tables=False, count=1, neq=0):
    """Which kernel form and which summation path a call takes, by the library's DEFAULT options.
      "eval" / "bind_eval"  sp_sumcheck_eval_batched / sp_sumcheck_bind_eval_batched at tables of `length`
      "bind2"               one trip of k_cubic_bind2_eval (eval_coeffs: nbind 0; bind2_eval*: nbind 1 or 2) at tables of `length` before its binds
      "tree"                sp_product_tree_many_from(.., count, n = length, 0)
      "eq"                  sp_sumcheck_*_batched_eq"""
    K = constants()
    if call in ("eval", "bind_eval"):
        work = length // 2 if call == "eval" else length // 4
        tiny = work <= TINY_MAX
        per_block = 64 if call == "eval" else 32          # k_cubic_eval_tiny: 64 indices per block; k_cubic_bind_eval_tiny: 32
        nblk = (work + per_block - 1) // per_block if tiny else _grid_for(work, 256)
        host = tiny and (nblk == 1 or 96 * nblk * ninst <= K["HOST_SUM_BYTES"])      # host_sums() && tiny
        return {"form": "tiny" if tiny else "streaming", "nblk": nblk, "sums": "host" if host else "kernel", "product": nblk * ninst,
                "args": "inline" if ninst <= INLINE_MAX_INST else "staged"}
    if call == "bind2":                                   # bind2_shape
        n2 = length >> nbind
        np_ = min(n2, 4)
        nblk = (n2 // np_ + 7) // 8
        host = 32 * 18 * nblk * ninst <= K["HOST_SUM_BYTES"]
        tail = want_tables and 2 <= n2 <= 8 and ninst <= K["TAIL_MAX_INST"] and host and nblk == 1
        return {"n2": n2, "nblk": nblk, "sums": "host" if host else "kernel", "tail": tail, "args": "inline" if ninst <= INLINE_MAX_INST else "staged"}
    if call == "tree":
        launches, ln = [], length
        while ln > 2:
            if ln <= TREE_TAIL_MAX:
                launches.append(("tail", ln))
                break
            if TREE_TWO_MIN <= ln <= (1 << TREE_TWO_MAX_LOG2):
                launches.append(("two", ln))
                ln //= 4
            else:
                launches.append(("one", ln))
                ln //= 2
        return {"launches": launches, "chunks": (count + TREE_CHUNK - 1) // TREE_CHUNK}
    if call == "eq":
        ok = length >= EQ_MIN_LEN and 1 <= neq <= ninst <= EQ_MAX_INST
        return {"ok": ok, "generic_launch": ok and ninst > neq}
    raise ValueError(call)
