"""Python-integer models of the F_q streaming kernels (spartan_amd/csrc/fq_ops.hip: the eq tables, the sum-check evaluate / bind kernels
of the ZK sum-checks, bind-top, vector x matrix, dot, evaluate, the gather / split / pack helpers) and a restatement of their host-side
dispatch arithmetic. Test infrastructure only: no GPU, no ctypes, no import of spartan_amd.

Every value is a RAW MONTGOMERY RESIDUE below q, as in tests/spark_reference.py, whose edge tables (layout a: neighbours differ; layout
c: runs of 64 equal values), challenge cycle (0, one, q - 1, random) and mm / bind / eq_table are reused here: the device's fq_mul is
mm(a, b) = a b R^-1 mod q, its fq_add / fq_sub are plain arithmetic mod q.

The models are written from the comments in fq_ops.hip and the reference lines they cite. Sums are accumulated as exact integers and
reduced once.

plan(...) restates which kernel form, how many blocks, which summation path, how many grid-stride passes and which challenge transport
a call takes. Its only purpose is to keep the case lists of tests/test_gpu_fq_edges.py on the boundaries of the dispatch
(tests/test_fq_reference.py checks that); it is never an expected value for device output."""
import os
from tests import spark_reference as S
from tests.helpers import Q, RINV, ROOT

ONE = S.ONE
RINV2 = S.RINV2
mm = S.mm
edge_table = S.edge_table
edge_challenges = S.edge_challenges
bind = S.bind              # bound_poly_var_top: T'[i] = T[i] + r (T[i + len/2] - T[i])  (dense_mlpoly.rs:215-223)
chi = S.eq_table           # EqPolynomial::evals (dense_mlpoly.rs:68-84): entry x = prod_k eq(x_k, r_k), r[0] the top variable

_POOL_BYTES = {}


def edge_table_bytes(layout, n, k):
    """the packed bytes of edge_table(layout, n, k) (32 little-endian bytes per residue) without making n Python integers"""
    pool = S.edge_pool()
    if "p" not in _POOL_BYTES:
        _POOL_BYTES["p"] = [x.to_bytes(32, "little") for x in pool]
    pb = _POOL_BYTES["p"]
    off = 977 * k % len(pool)
    rot = pb[off:] + pb[:off]
    if layout == "a":
        one = b"".join(rot)
        return (one * (n // len(rot) + 1))[:32 * n]
    one = b"".join(e * 64 for e in rot)
    return (one * (n // (64 * len(rot)) + 1))[:32 * n]


# ------------------------------------------------------------------ the sum-check kinds 0 (A B), 1 (A B C), 2 (A (B C - D))
NTABS = {0: 2, 1: 3, 2: 4}
POINTS = {0: (0, 2), 1: (0, 2, 3), 2: (0, 2, 3)}      # the evaluation points a kind returns


def _line(T, t):
    """the line through (0, T[i]), (1, T[i + len/2]) at the integer t, for every i (not reduced)"""
    h = len(T) // 2
    if t == 0:
        return T[:h]
    return [u + t * (v - u) for u, v in zip(T[:h], T[h:])]


def sc_evals(kind, tabs):
    """sum_i comb(A(t), B(t), ..) over the top-variable pairs (i, i + len/2) at t = 0, 2 (kind 0) or 0, 2, 3 (sumcheck.rs:460-469, 203-228,
    624-652; sc_point). mm(a, mm(b, c) - d) = a b c R^-2 - a d R^-1."""
    out = []
    for t in POINTS[kind]:
        L = [_line(T, t) for T in tabs]
        if kind == 0:
            out.append(sum(a * b for a, b in zip(L[0], L[1])) * RINV % Q)
        elif kind == 1:
            out.append(sum(a * b * c for a, b, c in zip(*L)) * RINV2 % Q)
        else:
            s3 = sum(a * b * c for a, b, c in zip(L[0], L[1], L[2]))
            s2 = sum(a * d for a, d in zip(L[0], L[3]))
            out.append((s3 * RINV2 - s2 * RINV) % Q)
    return out


def sc_term(kind, tabs, i, t):
    """the single term that index i contributes to the sum at the point t"""
    h = len(tabs[0]) // 2
    v = [T[i] + t * (T[h + i] - T[i]) for T in tabs]
    if kind == 0:
        return v[0] * v[1] * RINV % Q
    if kind == 1:
        return v[0] * v[1] * v[2] * RINV2 % Q
    return (v[0] * v[1] * v[2] * RINV2 - v[0] * v[3] * RINV) % Q


def bound_pair(T, r, i):
    """entries i and i + len/4 of bind(T, r) from the four entries the fused kernels read (x0, x1, x2, x3 at i + {0, 1, 2, 3} len/4)"""
    q4 = len(T) // 4
    rc = r * RINV % Q
    return (T[i] + rc * (T[i + 2 * q4] - T[i])) % Q, (T[i + q4] + rc * (T[i + 3 * q4] - T[i + q4])) % Q


def sc_bound_term(kind, tabs, r, i, t):
    """the term of index i < len/4 in the evaluation at t that follows a bind at r"""
    v = []
    for T in tabs:
        lo, hi = bound_pair(T, r, i)
        v.append(lo + t * (hi - lo))
    if kind == 0:
        return v[0] * v[1] * RINV % Q
    if kind == 1:
        return v[0] * v[1] * v[2] * RINV2 % Q
    return (v[0] * v[1] * v[2] * RINV2 - v[0] * v[3] * RINV) % Q


# ------------------------------------------------------------------ the linear kernels
def vecmat(L, Z, R):
    """DensePolynomial::bound (dense_mlpoly.rs:206-213): out[i] = sum_j L[j] Z[j R + i], Z viewed as len(L) x R"""
    acc = [0] * R
    for j, lj in enumerate(L):
        if lj:
            acc = [a + lj * z for a, z in zip(acc, Z[j * R:(j + 1) * R])]
    return [a * RINV % Q for a in acc]


def dot(a, b):
    return sum(x * y for x, y in zip(a, b)) * RINV % Q


def dot_term(a, b, i):
    return a[i] * b[i] * RINV % Q


def evaluate(Z, r):
    """DensePolynomial::evaluate (dense_mlpoly.rs:236-242): <Z, chi(r)>"""
    return dot(Z, chi(r))


def chi_at(r, i):
    """entry i of chi(r) alone"""
    ell, acc = len(r), ONE
    for k, rk in enumerate(r):
        acc = mm(acc, rk if (i >> (ell - 1 - k)) & 1 else (ONE - rk) % Q)
    return acc


# ------------------------------------------------------------------ the index maps of the copy kernels
def residue_split(src, W, g):
    """dst[k] = src[k W + g]"""
    return [src[k * W + g] for k in range(len(src) // W)]


def pack(tabs, count):
    """out[t count + e] = tabs[t][e]"""
    return [T[e] for T in tabs for e in range(count)]


def unpack_residues(buf, ntabs, W, sub):
    """in[(g ntabs + t) sub + k] -> tab[t][k W + g]"""
    tabs = [[None] * (W * sub) for _ in range(ntabs)]
    for g in range(W):
        for t in range(ntabs):
            for k in range(sub):
                tabs[t][k * W + g] = buf[(g * ntabs + t) * sub + k]
    return tabs


def gather(tabs, offs, count):
    """out[k count + e] = tabs[k][offs[k] + e]"""
    return [T[o + e] for T, o in zip(tabs, offs) for e in range(count)]


def tagged(n, tag):
    """n distinct residues that carry their table's tag and their own index: a copy from a wrong index or a wrong table cannot compare
    equal (the edge pool repeats)"""
    return [((tag + 1) << 200) | ((i + 1) << 64) | (0x9E3779B97F4A7C15 * (i + 1) & 0xFFFFFFFFFFFFFFFF) for i in range(n)]


# ------------------------------------------------------------------ the dispatch arithmetic, restated
_CONST = {}


def constants():
    """the named constants, read from the source as spark_reference.constants() does: a renamed or re-expressed one raises"""
    if not _CONST:
        c = S._constant
        _CONST.update(HOST_SUM_BYTES=c("internal.hpp", "HOST_SUM_BYTES"), HMAP_IN=c("internal.hpp", "HMAP_IN"), HMAP_SIZE=c("internal.hpp", "HMAP_SIZE"),
                      EQ_SLOTS=c("internal.hpp", "EQ_SLOTS"), EQ_SMALL_ELL=c("fq_ops.hip", "EQ_SMALL_ELL"), EQ_TOPB=c("fq_ops.hip", "EQ_TOPB"))
    return _CONST


# the thresholds that fq_ops.hip writes as literals, each with the text it must still contain (tests/test_fq_reference.py looks for it)
ONE_BLOCK_HALF = 256       # sp_sumcheck_eval
TINY_MAX_QUARTER = 8192    # sp_sumcheck_bind_eval and its _start / _commit forms; kind 1 has no tiny form
TINY_PER_BLOCK = 32        # k_sc_bind_eval_tiny: 32 indices x 8 lanes
GRID_MAX = 1024            # grid_for(.., 1024) of the summing kernels
VECMAT_SWITCH = 1 << 22    # vecmat_jchunk
EQ_MAX_ELL = 32            # sp_eq_expand
EQ_INLINE_MAX = 13         # struct EqR, launch_eq_small
EQ_SMALL_R = 16            # k_eq_expand_small: __shared__ Fq r[16]
SOURCE_TEXT = [
    "nblk = half <= 256 ? 1 : grid_for(half, 1024)",
    "bool tiny = kind != 1 && quarter <= 8192;",
    "size_t nblk = tiny ? (quarter + 31) / 32 : grid_for(quarter, 1024);",
    "Fq* partials = tiny ? partials_dst(c, nblk, 3) : (Fq*)c->scratch;",
    "size_t nblk = grid_for(n, 1024);",
    "nblk = grid_for(nthreads, 1024);",
    "return Lsz * R <= ((size_t)1 << 22) ? 16 : 32;",
    "ell == 0 || ell > 32",
    "struct EqR { Fq r[13]; };",
    "inline_args && r_host && ell <= 13",
    "__shared__ Fq r[16];",
    "size_t hi_ell = ell - ell / 2, lo_ell = ell / 2",
    "__shared__ Fq sm[8][32];",
    "dim3((unsigned)((R + 63) / 64), (unsigned)nchunks)",
    "8 * ntabs > HMAP_GEN || 32 * ntabs > HMAP_SIZE - HMAP_IN",
    "32 * ntabs * count > HMAP_SIZE - HMAP_IN",
]
# the shape of a single sum-check round is planned in ONE place (eval_plan, round_plan and plan_sums): sp_sumcheck_eval's block count, the
# tiny threshold, the bind-and-evaluate block count and the _start placement rule. A second copy of one of them could drift unnoticed
SOURCE_TEXT_ONCE = SOURCE_TEXT[:4]


def _source():
    return open(os.path.join(ROOT, "spartan_amd", "csrc", "fq_ops.hip")).read()


def source_text_missing():
    """the entries of SOURCE_TEXT that fq_ops.hip no longer contains"""
    src = _source()
    return [t for t in SOURCE_TEXT if t not in src]


def source_text_counts():
    """how often fq_ops.hip contains each entry of SOURCE_TEXT_ONCE"""
    src = _source()
    return {t: src.count(t) for t in SOURCE_TEXT_ONCE}


def _grid_for(work, maxblocks=2048):
    return max(1, min(maxblocks, (work + 255) // 256))     # internal.hpp, grid_for


def _sums(nblk, K, per_block, work):
    """partials_dst: up to HOST_SUM_BYTES of partial sums go to the host page; grid-stride passes of 256-thread blocks"""
    host = 32 * nblk * K <= constants()["HOST_SUM_BYTES"]
    return {"nblk": nblk, "block": per_block, "sums": "host" if host else "device", "passes": (work + nblk * per_block - 1) // (nblk * per_block),
            "work": work}


def plan(call, length=0, kind=0, start=False, ell=0, inline_args=1, Lsz=0, R=0, ntabs=0, count=1):
    """By the library's default options (inline_args: the option sumcheck.inline_args):
      "sc_eval"       sp_sumcheck_eval on tables of `length`
      "sc_bind_eval"  sp_sumcheck_bind_eval / _commit (start: sp_sumcheck_bind_eval_start) on tables of `length`
      "dot"           sp_dot over n = length
      "evaluate"      sp_evaluate at ell
      "vecmat"        sp_vecmat* with Lsz rows of R
      "eq"            sp_eq_expand at ell
      "heads"         sp_table_bind_top_heads / sp_table_heads / sp_table_gather: whether ntabs * count fits the result area"""
    K = constants()
    if call == "sc_eval":
        half = length // 2
        nblk = 1 if half <= ONE_BLOCK_HALF else _grid_for(half, GRID_MAX)
        p = _sums(nblk, 3, 256, half)
        p["form"] = "one block" if nblk == 1 else "streaming"
        return p
    if call == "sc_bind_eval":
        quarter = length // 4
        tiny = kind != 1 and quarter <= TINY_MAX_QUARTER
        nblk = (quarter + TINY_PER_BLOCK - 1) // TINY_PER_BLOCK if tiny else _grid_for(quarter, GRID_MAX)
        p = _sums(nblk, 3, TINY_PER_BLOCK if tiny else 256, quarter)
        if start and not tiny:
            p["sums"] = "device"      # _start: the streaming form always goes through k_reduce_partials
        p["form"] = "tiny" if tiny else "streaming"
        p["live"] = quarter - (nblk - 1) * p["block"] if p["passes"] == 1 else p["block"]      # live indices of the last block
        return p
    if call == "dot":
        return _sums(_grid_for(length, GRID_MAX), 1, 256, length)
    if call == "evaluate":
        topb = min(ell, K["EQ_TOPB"])
        nthreads = (1 << ell) >> topb
        p = _sums(_grid_for(nthreads, GRID_MAX), 1, 256, nthreads)
        p["topb"] = topb
        return p
    if call == "vecmat":
        jchunk = 16 if Lsz * R <= VECMAT_SWITCH else 32
        nchunks = (Lsz + jchunk - 1) // jchunk
        return {"jchunk": jchunk, "nchunks": nchunks, "last_chunk_rows": Lsz - (nchunks - 1) * jchunk, "col_blocks": (R + 63) // 64,
                "colsum_blocks": (R + 31) // 32, "colsum_wraps": nchunks > 8}
    if call == "eq":
        if ell < 1 or ell > EQ_MAX_ELL:
            return {"ok": False}
        small = lambda e: {"ell": e, "args": "inline" if inline_args and e <= EQ_INLINE_MAX else "staged", "nlo": min(e, 8), "nhi": e - min(e, 8),
                           "blocks": ((1 << e) + 255) // 256}
        if ell <= K["EQ_SMALL_ELL"]:
            return {"ok": True, "form": "small", "parts": [small(ell)]}
        hi, lo = ell - ell // 2, ell // 2
        assert hi <= EQ_SMALL_R
        return {"ok": True, "form": "outer", "parts": [small(hi), small(lo)]}
    if call == "heads":
        return {"ok": 32 * ntabs * count <= K["HMAP_SIZE"] - K["HMAP_IN"]}
    raise ValueError(call)


def boundary_indices(p):
    """the indices of a summing call whose terms no compared sum may be blind to: 0, the last index of the first block, the first of the
    second, the last index, and the first index of the second grid-stride pass"""
    w, b = p["work"], p["block"]
    idx = {0, w - 1}
    if p["nblk"] > 1:
        idx |= {b - 1, b}
    if p["passes"] > 1:
        idx.add(p["nblk"] * b)
    return sorted(i for i in idx if 0 <= i < w)
