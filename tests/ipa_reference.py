"""Python-integer model of the inner-product argument (spartan_amd/csrc/ipa.hip; k_ipa_round and ipa_round_launch in commit.hip) for
tests/test_ipa_reference.py (CPU) and tests/test_gpu_ipa_edges.py: the algebra of BulletReductionProof::prove (nizk/bullet.rs:32-132) in the
two forms the project relies on, the signed window digits of msm.hpp, the edge-value pools, and the host state machine's dispatch restated
(plan / trace). Python integers only: no device, and ctypes only to call the oracle handle a function is given.

  IpaModel            a, b, the coefficient vector s over the ORIGINAL generators (include/spartan_hip.h: the folded generator G'[i] is
                      sum_p s[p] G[p n_cur + i], so every L, R, g_hat is a fixed-base row with scalars s (x) a)
  folded_reference    the reference's own algorithm: G folded every round, every point through orc_pt_msm
  flat_reference      the same bytes from the model's flat rows (licensed by tests/test_ipa_reference.py; used where folding G is too slow)
  Geom / digits       msm_geom, msm_geom_windows, msm_bitpos, msm_digit
  plan / trace        which kernels a call runs, on what grid, and what it leaves behind"""
import os, re
from tests.helpers import Q, ROOT, mont_bulk, sz, rand_scalars

INV = lambda x: pow(x, Q - 2, Q)
NEUTRAL = bytes(32)      # RFC 9496 encoding of the neutral element


# ------------------------------------------------------------------ the script of one argument
def make_script(n0, rng, q_scale=None, zero_blinds=False, u=None, d=None, r=None, double_fold_at=None):
    """Everything the caller of sp_ipa_* supplies besides the vectors, drawn in the order the helper of tests/test_gpu_large.py always drew it
    (q_scale; per round blind_L, blind_R, u; then d, r). steps: ("round", blind_L, blind_R) | ("fold", u, u_inv).
    u: one challenge for every round instead of random ones. double_fold_at: the (1-based) round after which TWO folds follow with no round
    between (the API allows it: ipa_flush_fold)."""
    qs = rng.getrandbits(250)
    steps, cur, k = [], n0, 0
    while cur > 1:
        k += 1
        bl, br = rng.getrandbits(250), rng.getrandbits(249)
        uu = rng.getrandbits(251) | 1
        if u is not None:
            uu = u
        steps.append(("round", 0 if zero_blinds else bl, 0 if zero_blinds else br))
        steps.append(("fold", uu, INV(uu)))
        cur //= 2
        if double_fold_at == k and cur > 1:
            u2 = rng.getrandbits(251) | 1
            steps.append(("fold", u2, INV(u2)))
            cur //= 2
    dd, rr = rng.getrandbits(250), rng.getrandbits(250)
    return {"q_scale": qs if q_scale is None else q_scale, "steps": steps, "d": dd if d is None else d, "r": rr if r is None else r}


def challenges(script):
    return [(s[1], s[2]) for s in script["steps"] if s[0] == "fold"]


# ------------------------------------------------------------------ the model
class IpaModel:
    def __init__(self, a, b, g_off=0, q_idx=None, h_idx=None, q_scale=1):
        assert len(a) == len(b) and len(a) >= 1 and len(a) & (len(a) - 1) == 0
        self.a, self.b, self.s = [x % Q for x in a], [x % Q for x in b], [1]
        self.n0 = self.n_cur = len(a)
        self.g_off, self.q_scale = g_off, q_scale % Q
        self.q_idx = g_off + self.n0 if q_idx is None else q_idx
        self.h_idx = g_off + self.n0 + 1 if h_idx is None else h_idx

    def round(self, blind_L, blind_R):
        """(c_L, c_R, row_L, row_R): bullet.rs:80-97 with generator j = p n_cur + i carrying the coefficient s[p]; a row is a flat list of
        (scalar, generator index) over the original generators, then c Q and blind H"""
        n, h, a, b, s, g0 = self.n_cur, self.n_cur // 2, self.a, self.b, self.s, self.g_off
        assert n >= 2
        cL = sum(a[i] * b[h + i] for i in range(h)) % Q
        cR = sum(a[h + i] * b[i] for i in range(h)) % Q
        rowL = [(a[i] * s[p] % Q, g0 + p * n + h + i) for p in range(self.n0 // n) for i in range(h)]
        rowR = [(a[h + i] * s[p] % Q, g0 + p * n + i) for p in range(self.n0 // n) for i in range(h)]
        rowL += [(cL * self.q_scale % Q, self.q_idx), (blind_L % Q, self.h_idx)]
        rowR += [(cR * self.q_scale % Q, self.q_idx), (blind_R % Q, self.h_idx)]
        return cL, cR, rowL, rowR

    def fold(self, u, u_inv):
        """bullet.rs:105-109; the G fold G'[i] = u^-1 G[i] + u G[h + i] becomes s'[2p] = s[p] u^-1, s'[2p+1] = s[p] u"""
        h, a, b = self.n_cur // 2, self.a, self.b
        assert self.n_cur >= 2
        self.a = [(a[i] * u + u_inv * a[h + i]) % Q for i in range(h)]
        self.b = [(b[i] * u_inv + u * b[h + i]) % Q for i in range(h)]
        self.s = [x for sp in self.s for x in (sp * u_inv % Q, sp * u % Q)]
        self.n_cur = h

    def ghat_row(self):
        assert self.n_cur == 1
        return [(self.s[j], self.g_off + j) for j in range(self.n0)]

    def finish(self, d, r):
        """(a_hat, b_hat, the scalar row of delta = d g_hat + r H; nizk/mod.rs:496-501) — the row keeps its 0 * Q column, as the device row does"""
        assert self.n_cur == 1
        return self.a[0], self.b[0], [(d * self.s[j] % Q, self.g_off + j) for j in range(self.n0)] + [(0, self.q_idx), (r % Q, self.h_idx)]


def _msm(orc, scalars, points):
    import ctypes
    out = (ctypes.c_uint8 * 32)()
    assert orc.orc_pt_msm(mont_bulk(scalars), b"".join(points), sz(len(points)), out) == 1
    return bytes(out)


def folded_reference(orc, P, a, b, script, g_off=0, q_idx=None, h_idx=None):
    """BulletReductionProof::prove as the reference computes it — G folded every round, L = <a_L, G_R> + c_L Q + blind_L H over the FOLDED
    generators — through the oracle's point arithmetic only. P: the compressed points of the whole set. Returns
    {"L": [...], "R": [...] (one per round), "a_hat", "b_hat", "g_hat", "delta"}."""
    n = len(a)
    q_idx = g_off + n if q_idx is None else q_idx
    h_idx = g_off + n + 1 if h_idx is None else h_idx
    a, b = [x % Q for x in a], [x % Q for x in b]
    Qp = _msm(orc, [script["q_scale"]], [P[q_idx]])           # gens_1.scale(r) (nizk/mod.rs:479-480)
    H = P[h_idx]
    G = list(P[g_off:g_off + n])
    out = {"L": [], "R": []}
    for st in script["steps"]:
        h = len(a) // 2
        if st[0] == "round":
            cL = sum(a[i] * b[h + i] for i in range(h)) % Q
            cR = sum(a[h + i] * b[i] for i in range(h)) % Q
            out["L"].append(_msm(orc, a[:h] + [cL, st[1]], G[h:] + [Qp, H]))      # bullet.rs:83-89
            out["R"].append(_msm(orc, a[h:] + [cR, st[2]], G[:h] + [Qp, H]))      # :91-97
        else:
            u, ui = st[1], st[2]
            a = [(a[i] * u + ui * a[h + i]) % Q for i in range(h)]                # :105-106
            b = [(b[i] * ui + u * b[h + i]) % Q for i in range(h)]
            G = [_msm(orc, [ui, u], [G[i], G[h + i]]) for i in range(h)]          # :108
    assert len(a) == 1
    out.update(a_hat=a[0], b_hat=b[0], g_hat=G[0], delta=_msm(orc, [script["d"], script["r"]], [G[0], H]))   # nizk/mod.rs:496-501
    return out


def run_model(a, b, script, g_off=0, q_idx=None, h_idx=None):
    """the model driven through a script: ({"rounds": [(c_L, c_R, row_L, row_R, state before)], "a_hat", "b_hat", "ghat_row", "delta_row"}, model)"""
    m = IpaModel(a, b, g_off, q_idx, h_idx, script["q_scale"])
    rounds = []
    for st in script["steps"]:
        if st[0] == "round":
            rounds.append(m.round(st[1], st[2]) + ({"n_cur": m.n_cur, "a": list(m.a), "b": list(m.b)},))
        else:
            m.fold(st[1], st[2])
    ah, bh, drow = m.finish(script["d"], script["r"])
    return {"rounds": rounds, "a_hat": ah, "b_hat": bh, "ghat_row": m.ghat_row(), "delta_row": drow}, m


def flat_reference(orc, P, a, b, script, g_off=0, q_idx=None, h_idx=None, max_rounds=None, threads=1):
    """the same dictionary as folded_reference from the model's flat rows: one orc_pt_msm per compared point, no folded generator.
    max_rounds: only the first rounds (a_hat, b_hat, g_hat, delta are then absent). threads: the rows are independent and the oracle call
    releases the interpreter lock, so a large opening may spread them over a few cores."""
    m = IpaModel(a, b, g_off, q_idx, h_idx, script["q_scale"])
    rows, k = [], 0
    for st in script["steps"]:
        if st[0] == "round":
            if k == max_rounds:
                break
            k += 1
            _, _, rl, rr = m.round(st[1], st[2])
            rows += [rl, rr]
        else:
            m.fold(st[1], st[2])
    out = {}
    if max_rounds is None:
        ah, bh, drow = m.finish(script["d"], script["r"])
        rows += [m.ghat_row(), drow]
        out.update(a_hat=ah, b_hat=bh)
    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            pts = list(ex.map(lambda r: _row(orc, P, r), rows))
    else:
        pts = [_row(orc, P, r) for r in rows]
    out.update(L=pts[0:2 * k:2], R=pts[1:2 * k:2])
    if max_rounds is None:
        out.update(g_hat=pts[2 * k], delta=pts[2 * k + 1])
    return out


def _row(orc, P, row):
    return _msm(orc, [s for s, _ in row], [P[j] for _, j in row])


# ------------------------------------------------------------------ window geometry and signed digits (msm.hpp)
class Geom:
    """msm_geom(wbits) (uniform) or msm_geom_windows(nwin) (the nwide top windows one bit wider)"""
    def __init__(self, wbits=0, windows=0):
        if wbits:
            self.wbits, self.nwin, self.nwide = wbits, (254 + wbits - 1) // wbits, 0
        else:
            self.nwin, self.wbits = windows, 254 // windows
            self.nwide = 254 - windows * self.wbits
        self.tent = 1 << (self.wbits - 1)
        self.n0 = self.nwin - self.nwide          # first wide window
        self.pt_entries = (self.nwin + self.nwide) * self.tent

    def width(self, w):
        return self.wbits + (1 if w >= self.n0 else 0)

    def bitpos(self, w):
        return w * self.wbits + (w - self.n0 if w > self.n0 else 0)

    def half(self, w):
        """the `tent` of window w: the digit that turns into a carry"""
        return 1 << (self.width(w) - 1)

    def field(self, s, w):
        return (s >> self.bitpos(w)) & ((1 << self.width(w)) - 1)

    def digits(self, s):
        """msm_digit for every window: d_w in [-half, half), carry chain from the bottom"""
        out, carry = [], 0
        for w in range(self.nwin):
            d = self.field(s, w) + carry
            carry = 1 if d >= self.half(w) else 0
            out.append(d - (carry << self.width(w)))
        assert carry == 0, "a scalar below 2^253 leaves no carry"
        return out

    def table_bytes(self, npoints):
        return npoints * self.pt_entries * 128


def edge_pool():
    """the scalar pool of helpers.rand_scalars(kind="edge"), once each"""
    class _Seq:      # draws index 0, 1, 2, ...: the pool itself, in its order, however long it is
        def __init__(self): self.k = -1
        def randrange(self, n):
            self.k += 1
            if self.k >= n:
                raise IndexError
            return self.k
    rng, out = _Seq(), []
    while True:
        try:
            out += rand_scalars(rng, 1, "edge")
        except IndexError:
            return out


def digit_pool(geom):
    """Scalars (< Q) for the carry chain of msm_digit under `geom`: per window w one whose field at msm_bitpos(w) is exactly the window's
    tent and one tent - 1 (all other bits clear: the digit is -tent with a carry out, resp. the largest positive digit), for narrow and wide
    windows alike; 2^253 - 1 mod Q; the largest value below 2^252 with every field 2^c - 1 (the carry born in window 0 runs to the top);
    and a carry that arrives at a window holding tent - 1 (it tips it over)."""
    out = []
    for w in range(geom.nwin):
        for f in (geom.half(w), geom.half(w) - 1):
            v = f << geom.bitpos(w)
            if 0 < v < Q:
                out.append(v)
        if w + 1 < geom.nwin:
            v = (geom.half(w) << geom.bitpos(w)) | ((geom.half(w + 1) - 1) << geom.bitpos(w + 1))
            if v < Q:
                out.append(v)
    out += [(2**253 - 1) % Q, 2**252 - 1, Q - 1]
    return out


def edge_vector(n, rng, pool=None):
    pool = pool or edge_pool()
    return [pool[rng.randrange(len(pool))] for _ in range(n)]


# ------------------------------------------------------------------ constructors for the value relations
def unfold(target, u, u_inv, left):
    """the vector one round earlier whose fold by (u, u^-1) is `target` and whose left half is `left`: a' = a_L u + u^-1 a_R"""
    assert len(target) == len(left) and u * u_inv % Q == 1
    return [x % Q for x in left] + [(t - l * u) * u % Q for t, l in zip(target, left)]


def a_reaching(n0, script, rounds_done, target, rng):
    """an `a` of length n0 that, after the first `rounds_done` folds of the script, IS `target` — with non-zero random left halves on the way,
    so a zero in target is a scalar that is zero only after the fold (a_R = -a_L u^2 at that index)"""
    ch = challenges(script)[:rounds_done]
    v = list(target)
    assert len(v) << rounds_done == n0
    for u, ui in reversed(ch):
        v = unfold(v, u, ui, [rng.randrange(1, Q) for _ in v])
    return v


def b_with_cL_zero(a, b):
    """b with its last entry set so that c_L = <a_L, b_R> = 0 in the first round (a[h - 1] must be non-zero)"""
    h = len(a) // 2
    b = list(b)
    if h == 0:
        return b
    assert a[h - 1] % Q
    b[2 * h - 1] = -sum(a[i] * b[h + i] for i in range(h - 1)) * INV(a[h - 1]) % Q
    return b


# ------------------------------------------------------------------ the dispatch, restated from the source text
_CSRC = os.path.join(ROOT, "spartan_amd", "csrc")
# (file, regular expression with one group per constant, names): the literal thresholds of the host state machine and the kernels
_PATTERNS = [
    ("ipa.hip", r"static unsigned ipa_c0_blocks\(size_t n\) \{ return \(unsigned\)\(\(n / 2 \+ (\d+)\) / (\d+)\); \}", ("C0_ROUND", "C0_PAIRS")),
    ("ipa.hip", r"const bool want_c0 = ipa_fused\(c\) && n >= 2 && !c->device_encode && nblk0 <= (\d+);", ("C0_MAX_BLOCKS",)),
    ("ipa.hip", r"return ipa_fused\(c\) && !c->device_encode && ipa->n_cur <= (\d+) && \(\(ipa->fold_pending && ipa->have_dots\) \|\| \(!ipa->fold_pending && ipa->have_c0\)\);",
     ("FUSED_MAX_N",)),
    ("ipa.hip", r"hipLaunchKernelGGL\(k_ipa_prepare, dim3\(\(unsigned\)\(\(ipa->n0 \+ (\d+)\) / (\d+) \+ 1\)\), dim3\((\d+)\)", ("PREP_ROUND", "PREP_PER_BLOCK", "PREP_THREADS")),
    ("commit.hip", r"A->nblk = \(unsigned\)\(\(P \+ (\d+)\) / (\d+)\);", ("LOOKUP_ROUND", "LOOKUPS_PER_BLOCK")),
    ("commit.hip", r"A->nd = \(unsigned\)\(\(qlen \+ (\d+)\) / (\d+)\);", ("DOT_ROUND", "DOT_PER_BLOCK")),
    ("commit.hip", r"for \(size_t k2 = t; k2 < A\.nblk; k2 \+= (\d+)\) \{", ("REDUCE_STRIDE",)),
    ("commit.hip", r"if \(DED\) pt10_tree_quad_ded\(sm, idf, A\.nblk < (\d+) \? A\.nblk : (\d+)\);", ("REDUCE_WIDTH", "REDUCE_WIDTH2")),
    ("tree.hpp", r"__device__ __forceinline__ void pt10_tree_quad_ded\(Pt10\* sm, unsigned char\* idf, size_t n\) \{(?s:.{0,900}?)int top = (\d+);\s*while \(top > 1 && \(size_t\)top >= n\) top >>= 1;",
     ("TREE_TOP",)),
]
# text the plan restates without a number in it
SOURCE_TEXT = {
    "ipa.hip": [
        "const unsigned nblk0 = ipa_c0_blocks(n) ? ipa_c0_blocks(n) : 1;",
        "if (off || !ipa->have_fin || !ipa->fold_pending || ipa->ctx->device_encode) return false;",
        "if (fq_is_zero(a0) || fq_is_zero(a1)) return false;",
        "if (ipa->pre || !ipa_round_fusable(ipa)) return SP_OK;",
        "if (ipa->pre || ipa_round_fusable(ipa)) return ipa_round_fused(ipa, blind_L, blind_R, L_out, R_out);",
        "ipa->have_c0 = ipa->have_dots = false;",
        "if (ipa->n_cur == 2) {",
        "if (ipa->n_cur >= 4) {",
        "ipa->have_dots = false;  // they described the vectors before this fold",
        "if (n == 1) { st_fq(a, ld_fq(a_src)); st_fq(b, ld_fq(b_src)); idx[0] = (uint32_t)g_off; }",
        "!is_pow2(n) || g_off + n > g->n || q_idx >= g->n || h_idx >= g->n) return SP_EINVAL;",
        "if (a_dev && a_dev->cap < n) return SP_EINVAL;",
    ],
    "commit.hip": [
        "const size_t P = (A->n0 / 2) * (size_t)g->geom.nwin;",
        "const size_t qlen = A->n_cur >= 4 ? A->n_cur / 4 : 1;",
        "const bool always_unified = c->opt.v[OPT_IPA_UNIFIED_TREE] != 0 || (!g->derived && !c->opt.v[OPT_IPA_DEDICATED_UPLOADED]);",
        "if (DED) pt10_tree_quad_ded(sm, idf, P - (size_t)blk * 256);",
        "if (A.n_cur == 2) { st_fq(A.dots_out + 8 + x, av); st_fq(A.dots_out + 10 + x, bv); }",
        "if (!fq_is_zero(sc)) {",
    ],
}
_CONST = {}


def constants():
    """the literal thresholds, read from ipa.hip, commit.hip and tree.hpp: a changed number changes every plan below (and
    tests/test_ipa_reference.py then finds a boundary uncovered); a re-expressed line raises"""
    if not _CONST:
        for fn, pat, names in _PATTERNS:
            src = open(os.path.join(_CSRC, fn)).read()
            m = re.search(pat, src)
            if not m:
                raise AssertionError("%s no longer contains /%s/: restate tests/ipa_reference.py" % (fn, pat))
            _CONST.update({k: int(v) for k, v in zip(names, m.groups())})
        K = _CONST
        assert K["C0_ROUND"] == K["C0_PAIRS"] - 1 and K["PREP_ROUND"] == K["PREP_PER_BLOCK"] - 1 and K["LOOKUP_ROUND"] == K["LOOKUPS_PER_BLOCK"] - 1
        assert K["DOT_ROUND"] == K["DOT_PER_BLOCK"] - 1 and K["REDUCE_WIDTH"] == K["REDUCE_WIDTH2"] == K["REDUCE_STRIDE"] == K["LOOKUPS_PER_BLOCK"]
        assert K["PREP_THREADS"] == K["PREP_PER_BLOCK"]
    return _CONST


def source_text_missing():
    out = []
    for fn, texts in SOURCE_TEXT.items():
        src = open(os.path.join(_CSRC, fn)).read()
        out += [(fn, t) for t in texts if t not in src]
    return out


DEFAULT_OPTS = {"fused": 1, "device_encode": 0, "finish_device": 0, "derived": True, "dedicated_uploaded": 0, "unified_tree": 0}


def tree_top(n):
    top = constants()["TREE_TOP"]
    while top > 1 and top >= n:
        top >>= 1
    return top


def plan_begin(n0, opts=DEFAULT_OPTS):
    K = constants()
    nblk0 = (n0 // 2 + K["C0_ROUND"]) // K["C0_PAIRS"] or 1
    return {"nblk0": nblk0, "want_c0": bool(opts["fused"]) and n0 >= 2 and not opts["device_encode"] and nblk0 <= K["C0_MAX_BLOCKS"], "n1_arm": n0 == 1}


def plan(n0, n_cur, nwin, opts=DEFAULT_OPTS, state=None):
    """one sp_ipa_round_lr at n_cur entries of an n0 opening on an nwin-window generator set. state: fold_pending, have_c0, have_dots
    (what the calls before left behind: trace() keeps it)."""
    K = constants()
    st = {"fold_pending": False, "have_c0": False, "have_dots": False}
    st.update(state or {})
    p = dict(plan_begin(n0, opts))
    fusable = bool(opts["fused"]) and not opts["device_encode"] and n_cur <= K["FUSED_MAX_N"] and (
        (st["fold_pending"] and st["have_dots"]) or (not st["fold_pending"] and st["have_c0"]))
    p.update(fusable=fusable, fold=1 if st["fold_pending"] else 0, n_cur=n_cur, last=n_cur == 2)
    if not fusable:
        p.update(prepare_grid=(n0 + K["PREP_ROUND"]) // K["PREP_PER_BLOCK"] + 1, leaves_dots=False, leaves_fin=False)
        return p
    P = (n0 // 2) * nwin
    nblk = (P + K["LOOKUP_ROUND"]) // K["LOOKUPS_PER_BLOCK"]
    qlen = n_cur // 4 if n_cur >= 4 else 1
    nd = (qlen + K["DOT_ROUND"]) // K["DOT_PER_BLOCK"]
    last_count = P - (nblk - 1) * K["LOOKUPS_PER_BLOCK"]
    red = min(nblk, K["REDUCE_WIDTH"])
    unified = bool(opts["unified_tree"]) or (not opts["derived"] and not opts["dedicated_uploaded"])
    p.update(P=P, nblk=nblk, qlen=qlen, nd=nd, grid=2 * nblk + nd, last_count=last_count, last_top=tree_top(last_count), full_blocks=nblk - 1 if last_count < 256 else nblk,
             reduce_count=red, reduce_top=tree_top(red), reduce_strided=nblk > K["REDUCE_STRIDE"], tree="unified" if unified else "dedicated",
             leaves_dots=n_cur >= 4, leaves_fin=n_cur == 2, dot_lanes_live=min(4, n_cur) if qlen == 1 else 4)
    return p


def trace(n0, nwin, steps, opts=DEFAULT_OPTS, order=("finish_commit", "finish", "commit_ghat"), a_last_zero=False):
    """the host state machine of ipa.hip over the calls of one argument: a list of events
       ("begin", plan_begin) ("round", plan) ("flush_fold", n_cur) ("finish_commit", "host" | "device", fold) ("finish", flushed) ("commit_ghat", flushed)
    a_last_zero: the last round's a' has a zero entry (ipa_finish_on_host gives up)."""
    ev = [("begin", plan_begin(n0, opts))]
    st = {"fold_pending": False, "have_c0": ev[0][1]["want_c0"], "have_dots": False}
    have_fin, n_cur = False, n0
    for s in steps:
        if s[0] == "round":
            p = plan(n0, n_cur, nwin, opts, st)
            ev.append(("round", p))
            st.update(fold_pending=False, have_c0=False, have_dots=p["leaves_dots"])
            if p["leaves_fin"]:
                have_fin = True
        else:
            if st["fold_pending"]:
                ev.append(("flush_fold", n_cur))
                st.update(fold_pending=False, have_dots=False)
            st["fold_pending"] = True
            n_cur //= 2
    assert n_cur == 1
    for call in order:
        if call == "finish_commit":
            host = not opts["finish_device"] and have_fin and st["fold_pending"] and not opts["device_encode"] and not a_last_zero
            ev.append(("finish_commit", "host" if host else "device", 1 if st["fold_pending"] else 0))
        else:
            ev.append((call, st["fold_pending"]))
            st["fold_pending"] = False
    return ev
