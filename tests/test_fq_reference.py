"""CPU checks of tests/fq_reference.py, the Python-integer models that tests/test_gpu_fq_edges.py compares the kernels of
spartan_amd/csrc/fq_ops.hip with: the models against the oracle on edge-value inputs (the degenerate challenges included), the coverage of
the GPU module's case lists (together they must reach every boundary of the library's dispatch arithmetic, on both sides where there are
two, so a changed constant that slides a case off its boundary fails here, without a GPU), and the condition that no compared sum is blind
to an index at a block, pass or table boundary: the single term each such index contributes is not zero."""
import ctypes
import pytest
from tests import field_vectors as V
from tests import fq_reference as F
from tests import spark_reference as S
from tests import test_gpu_fq_edges as G      # the case lists and the pure-Python case builders: the binding is imported inside its tests
from tests.helpers import Q, R, sz, u64x4


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals))).from_buffer_copy(V.pack(vals))


def _ints(arr, n=None):
    raw = bytes(arr)
    n = len(raw) // 32 if n is None else n
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


# ------------------------------------------------------------------ the inputs
def test_the_packed_edge_tables_are_the_edge_tables():
    for layout in "ac":
        for n, k in ((1, 0), (63, 1), (64, 2), (65, 3), (3000, 5), (200000, 77)):
            assert F.edge_table_bytes(layout, n, k) == V.pack(F.edge_table(layout, n, k)), (layout, n, k)
    for kind, layout, n, base in ((0, "a", 2, 3), (2, "c", 256, 9), (1, "a", 4, 1)):
        T = G.case_tables(kind, layout, n, base)
        assert [V.pack(t) for t in T] == G.case_tables_raw(kind, layout, n, base)
        assert len(T) == F.NTABS[kind] and (n < 4 or T[1][:n // 2] == T[1][n // 2:])
    t = F.tagged(1025, 3) + F.tagged(1025, 4)
    assert len(set(t)) == 2050 and max(t) < Q


def test_the_challenge_vectors_hold_what_their_names_say():
    for ell in (1, 5, 17):
        v = {k: G.challenge_vector(k, ell) for k in G.EQ_VECTORS + ["dense"]}
        assert set(v["zero"]) == {0} and set(v["one"]) == {R % Q} and set(v["minus"]) == {Q - 1}
        assert v["cycle"][:3] == [0, R % Q, Q - 1][:ell] and not {0, R % Q} & set(v["dense"]) and Q - 1 in v["dense"]
        assert all(0 <= x < Q for vec in v.values() for x in vec)
    assert len({tuple(G.challenge_vector("random", 14, seed=100 + k)) for k in range(G.EQ_RING_CALLS)}) == G.EQ_RING_CALLS


# ------------------------------------------------------------------ the models against the oracle
@pytest.mark.parametrize("ell", [1, 2, 7, 9])
def test_chi_matches_the_oracle_on_every_kind_of_challenge_vector(orc, ell):
    for kind in G.EQ_VECTORS + ["dense"]:
        r = G.challenge_vector(kind, ell)
        o = (ctypes.c_uint64 * (4 << ell))()
        orc.orc_eq_evals(_arr(r), sz(ell), o)
        chi = F.chi(r)
        assert chi == _ints(o), (kind, ell)
        assert [F.chi_at(r, i) for i in range(1 << ell)] == chi
        if kind in ("zero", "one"):      # one-hot
            hot = 0 if kind == "zero" else (1 << ell) - 1
            assert chi == [F.ONE if i == hot else 0 for i in range(1 << ell)]


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("n", [2, 4, 64, 1024])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_sumcheck_models_match_the_oracle_on_edge_tables(orc, kind, n, layout):
    T = G.case_tables(kind, layout, n, 5 * kind)
    nv = len(F.POINTS[kind])

    def oracle(tabs):
        a = [_arr(t) for t in tabs] + [None] * (4 - len(tabs))
        w = (ctypes.c_uint64 * 12)()
        orc.orc_sumcheck_eval(ctypes.c_int(kind), a[0], a[1], a[2], a[3], sz(len(tabs[0])), w)
        return _ints(w, nv)

    assert F.sc_evals(kind, T) == oracle(T)
    h = n // 2
    for j, t in enumerate(F.POINTS[kind]):      # the single terms add up to the sum
        assert sum(F.sc_term(kind, T, i, t) for i in range(h)) % Q == F.sc_evals(kind, T)[j]
    for r in F.edge_challenges(n + kind):
        B = []
        for t in T:
            z = _arr(t)
            orc.orc_bound_top(z, sz(n), _arr([r]))
            B.append(F.bind(t, r))
            assert B[-1] == _ints(z, h), (hex(r), kind, n, layout)
        if n >= 4:
            assert F.sc_evals(kind, B) == oracle(B)
            for i in (0, n // 4 - 1):
                assert [F.bound_pair(t, r, i) for t in T] == [(b[i], b[n // 4 + i]) for b in B]
                for t in F.POINTS[kind]:
                    assert F.sc_bound_term(kind, T, r, i, t) == F.sc_term(kind, B, i, t)


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("nv", [1, 2, 7, 10])
def test_linear_models_match_the_oracle_on_edge_tables(orc, nv, layout):
    n = 1 << nv
    Z, W = F.edge_table(layout, n, 30), F.edge_table("a", n, 31)
    o = u64x4(); orc.orc_dot(_arr(Z), _arr(W), sz(n), o)
    assert [F.dot(Z, W)] == _ints(o)
    assert sum(F.dot_term(Z, W, i) for i in range(n)) % Q == F.dot(Z, W)
    Ls = 1 << (nv // 2); cols = n // Ls
    for Lv in (F.edge_table("a", Ls, 32), ([0, F.ONE, Q - 1] * Ls)[:Ls]):
        o = (ctypes.c_uint64 * (4 * cols))(); orc.orc_bound_vecmat(_arr(Z), sz(nv), _arr(Lv), o)
        assert F.vecmat(Lv, Z, cols) == _ints(o), (nv, layout)
    for kind in G.EVAL_VECTORS + ["zero", "one"]:      # evaluate: the dot with the oracle's own chi table
        r = G.challenge_vector(kind, nv)
        c = (ctypes.c_uint64 * (4 * n))(); orc.orc_eq_evals(_arr(r), sz(nv), c)
        o = u64x4(); orc.orc_dot(_arr(Z), c, sz(n), o)
        assert [F.evaluate(Z, r)] == _ints(o), (kind, nv)
    assert F.evaluate(Z, [0] * nv) == Z[0] and F.evaluate(Z, [F.ONE] * nv) == Z[-1]


def test_the_index_maps():
    src = list(range(100, 112))
    assert F.residue_split(src, 3, 1) == [101, 104, 107, 110] and F.residue_split(src, 1, 0) == src and F.residue_split(src, 12, 11) == [111]
    a, b = [1, 2, 3], [4, 5, 6]
    assert F.pack([a, b], 2) == [1, 2, 4, 5]
    assert F.gather([a, b], [1, 0], 2) == [2, 3, 4, 5]
    # in[(g ntabs + t) sub + k] -> tab[t][k W + g], W = 2, sub = 3, two tables
    assert F.unpack_residues([0, 1, 2, 10, 11, 12, 3, 4, 5, 13, 14, 15], 2, 2, 3) == [[0, 3, 1, 4, 2, 5], [10, 13, 11, 14, 12, 15]]
    for W in (1, 3, 4, 12):      # split, pack in shard order, unpack: the identity
        tabs = [F.tagged(12, 1), F.tagged(12, 2)]
        buf = [x for g in range(W) for x in F.pack([F.residue_split(t, W, g) for t in tabs], 12 // W)]
        assert F.unpack_residues(buf, 2, W, 12 // W) == tabs


# ------------------------------------------------------------------ the dispatch arithmetic
def test_the_constants_and_the_literal_thresholds_are_still_in_the_source():
    K = F.constants()
    assert set(K) == {"HOST_SUM_BYTES", "HMAP_IN", "HMAP_SIZE", "EQ_SLOTS", "EQ_SMALL_ELL", "EQ_TOPB"} and all(isinstance(v, int) and v > 0 for v in K.values())
    assert F.source_text_missing() == []
    assert len(F.SOURCE_TEXT) >= 16 and len(F.SOURCE_TEXT_ONCE) == 4 and "half <= 256" in F.SOURCE_TEXT_ONCE[0] and "(Fq*)c->scratch" in F.SOURCE_TEXT_ONCE[3]
    for text, count in F.source_text_counts().items():      # the plan of a single round stands once: `in` would pass while one of three copies is right
        assert count == 1, (text, count)
    assert K["EQ_SMALL_ELL"] <= F.EQ_INLINE_MAX and F.EQ_MAX_ELL - F.EQ_MAX_ELL // 2 == F.EQ_SMALL_R      # 32 is the last ell whose upper half fits r[16]
    assert (F.EQ_MAX_ELL + 1) - (F.EQ_MAX_ELL + 1) // 2 > F.EQ_SMALL_R


def _chain_calls():
    """every call the chain test makes: (call, kind, length, start) and the tables and challenge it is made with"""
    for kind, len0, layout, base, cstart in G.CHAIN_CASES:
        rounds = G.chain_model(kind, len0, layout, base, cstart)
        for j in range(len(rounds) - 1):
            T = rounds[j][1]
            yield ("sc_eval", kind, len(T[0]), False), T, None
            if len(T[0]) >= 4:
                for start in (False, True):
                    yield ("sc_bind_eval", kind, len(T[0]), start), T, rounds[j + 1][0]


def _round_calls():
    for call, kind, length, layout, base, ridx, _ in G.ROUND_CASES:
        yield (call, kind, length, False), (kind, layout, length, base), None if ridx is None else G.case_r(length, kind, ridx)
    for kind, length, rows, layout, base, ridx in G.COMMIT_CASES:
        yield ("sc_bind_eval", kind, length, False), (kind, layout, length, base), G.case_r(length, kind, ridx)


def _plan(key):
    call, kind, length, start = key
    return F.plan(call, length, kind, start)


def test_the_gpu_case_lists_reach_every_dispatch_boundary():
    K = F.constants()
    lim3, lim1 = K["HOST_SUM_BYTES"] // 96, K["HOST_SUM_BYTES"] // 32      # blocks whose sums the host still adds: 320 with K = 3, 960 with K = 1
    assert (lim3, lim1) == (320, 960)
    chain = {key: _plan(key) for key, _, _ in _chain_calls()}
    single = {key: _plan(key) for key, _, _ in _round_calls()}
    # --- the fused bind: tiny from quarter 8192 (256 blocks) down to one partly live block, streaming above, kind 1 streaming at every length
    for kind in (0, 2):
        mine = {k: p for k, p in chain.items() if k[0] == "sc_bind_eval" and k[1] == kind and not k[3]}
        assert any(p["form"] == "streaming" and p["work"] == 2 * F.TINY_MAX_QUARTER for p in mine.values()), kind
        assert any(p["form"] == "tiny" and p["work"] == F.TINY_MAX_QUARTER and p["nblk"] == 256 for p in mine.values()), kind
        assert {p["work"] for p in mine.values() if p["form"] == "tiny"} == {1 << e for e in range(14)}, kind
        assert any(p["nblk"] == 1 and p["live"] == F.TINY_PER_BLOCK for p in mine.values()) and any(p["nblk"] == 1 and p["live"] == 1 for p in mine.values())
        assert any(p["nblk"] == 2 for p in mine.values())
    k1 = [p for k, p in chain.items() if k[0] == "sc_bind_eval" and k[1] == 1]
    assert {p["form"] for p in k1} == {"streaming"} and {p["work"] for p in k1} == {1 << e for e in range(11)}
    assert any(p["work"] == F.TINY_MAX_QUARTER and p["form"] == "tiny" for k, p in single.items() if k[1] == 2)      # the round body with 8 rows
    # --- _start: tiny rounds host-summed, streaming rounds always through k_reduce_partials
    st = [p for k, p in chain.items() if k[0] == "sc_bind_eval" and k[3]]
    assert any(p["form"] == "tiny" and p["sums"] == "host" for p in st) and any(p["form"] == "streaming" and p["sums"] == "device" for p in st)
    assert not any(p["form"] == "tiny" and p["sums"] == "device" for p in chain.values() if "form" in p)      # 256 blocks at the most
    # --- _commit: a tiny plan and a streaming plan whose sums the host adds, and a streaming plan that goes through k_reduce_partials
    cm = [F.plan("sc_bind_eval", n, k) for k, n, *_ in G.COMMIT_CASES]
    for form, sums in (("tiny", "host"), ("streaming", "host"), ("streaming", "device")):
        assert any(p["form"] == form and p["sums"] == sums for p in cm), (form, sums)
    assert any(p["sums"] == "device" and p["nblk"] == 512 and 96 * p["nblk"] > K["HOST_SUM_BYTES"] for p in cm)
    # --- sp_sumcheck_eval: one block up to half = 256, then 256 indices per block
    ev = {k[2]: p for k, p in chain.items() if k[0] == "sc_eval" and k[1] == 0}
    assert ev[2 * F.ONE_BLOCK_HALF]["form"] == "one block" and ev[4 * F.ONE_BLOCK_HALF]["nblk"] == 2 and ev[2]["work"] == 1
    # --- the host-sum limit, both sides, every kind and both calls; one pass
    for kind in (0, 1, 2):
        for call in ("sc_eval", "sc_bind_eval"):
            mine = [p for k, p in single.items() if k[0] == call and k[1] == kind and p["passes"] == 1 and p["form"] == "streaming"]
            assert any(p["sums"] == "host" and lim3 // 2 < p["nblk"] <= lim3 for p in mine), (call, kind)      # the largest power of two at or below the limit
            assert any(p["sums"] == "device" and lim3 < p["nblk"] <= 2 * lim3 for p in mine), (call, kind)     # ... and the smallest above it
    # --- the second grid-stride pass, kind 0, both calls; one block count below the cap makes one pass
    for call in ("sc_eval", "sc_bind_eval"):
        mine = [p for k, p in single.items() if k[0] == call and k[1] == 0]
        assert any(p["passes"] == 2 and p["nblk"] == F.GRID_MAX and p["work"] == 2 * 256 * F.GRID_MAX for p in mine), call
        assert all(p["passes"] == 1 for p in mine if p["work"] <= 256 * F.GRID_MAX) and any(p["nblk"] == F.GRID_MAX // 2 for p in mine), call
    assert {src for *_, src in G.ROUND_CASES} == {"model", "oracle"} and [c[2] for c in G.ROUND_CASES if c[6] == "oracle"] == [1 << 21]
    # --- dot
    dots = {n: F.plan("dot", n) for n in G.DOT_N}
    assert dots[256]["nblk"] == 1 and dots[257]["nblk"] == 2
    assert dots[256 * lim1]["nblk"] == lim1 and dots[256 * lim1]["sums"] == "host" and dots[256 * lim1 + 1]["nblk"] == lim1 + 1 and dots[256 * lim1 + 1]["sums"] == "device"
    top = 256 * F.GRID_MAX
    assert dots[top]["passes"] == 1 and dots[top]["nblk"] == F.GRID_MAX and dots[top + 1]["passes"] == 2 and dots[top + 1]["nblk"] == F.GRID_MAX
    assert all(a and b for a, b in [G.DOT_OFF])
    # --- evaluate: every TOPB instantiation with one thread, TOPB = 4 with two, one full block, two blocks
    evs = {ell: F.plan("evaluate", ell=ell) for ell in G.EVAL_ELLS}
    assert [evs[e]["topb"] for e in (1, 2, 3, 4)] == [1, 2, 3, 4] and all(evs[e]["work"] == 1 for e in (1, 2, 3, 4)) and evs[5]["work"] == 2
    assert any(p["work"] == 256 and p["nblk"] == 1 for p in evs.values()) and any(p["work"] == 512 and p["nblk"] == 2 for p in evs.values())
    # --- vecmat
    vm = {c: F.plan("vecmat", Lsz=c[0], R=c[1]) for c in G.VECMAT_CASES}
    assert {8, 9} <= {p["nchunks"] for p in vm.values()} and {p["colsum_wraps"] for p in vm.values()} == {False, True}
    assert any(c[0] * c[1] == F.VECMAT_SWITCH and p["jchunk"] == 16 for c, p in vm.items())
    big = [(c, p) for c, p in vm.items() if p["jchunk"] == 32]
    assert big and all(F.VECMAT_SWITCH < c[0] * c[1] < F.VECMAT_SWITCH * 1.001 and c[0] % 32 and c[1] % 64 and p["last_chunk_rows"] != 32 for c, p in big)
    assert any(p["last_chunk_rows"] not in (16, 32) and p["nchunks"] > 1 for p in vm.values()) and any(c[0] < 4 for c in vm)      # fewer rows than row lanes
    assert any(c[1] % 64 == 0 for c in vm) and any(c[1] % 64 and c[1] % 32 == 0 for c in vm) and any(c[1] % 32 for c in vm) and any(c[1] < 32 for c in vm)
    assert set(G.VECMAT_DEV_CASES) <= set(G.VECMAT_CASES) and len(G.VECMAT_DEV_CASES) == 2
    # --- eq: both challenge transports at every ell, every count of high bits of the short kernel, outer products, the bound
    for inline in (1, 0):
        ps = {ell: F.plan("eq", ell=ell, inline_args=inline) for ell in G.EQ_ELLS}
        assert all(p["ok"] for p in ps.values())
        assert {a["args"] for p in ps.values() for a in p["parts"]} == ({"inline"} if inline else {"staged"})
        small = {ell: p["parts"][0] for ell, p in ps.items() if p["form"] == "small"}
        assert sorted(small) == list(range(1, K["EQ_SMALL_ELL"] + 1)) and {a["nhi"] for a in small.values()} == {0, 1, 2, 3, 4, 5}
        assert small[8]["nhi"] == 0 and small[9]["nhi"] == 1 and small[1]["nlo"] == 1 and small[2]["nlo"] == 2 and small[7]["nlo"] == 7
        outer = {ell: [a["ell"] for a in p["parts"]] for ell, p in ps.items() if p["form"] == "outer"}
        assert outer == {14: [7, 7], 15: [8, 7], 17: [9, 8]}
    assert G.EQ_RING_ELL > K["EQ_SMALL_ELL"] and G.EQ_RING_CALLS > K["EQ_SLOTS"]
    # the ring is read only by staged launches: on the inline_args = 0 context of the ring test both halves are, by default neither
    assert {a["args"] for a in F.plan("eq", ell=G.EQ_RING_ELL, inline_args=0)["parts"]} == {"staged"}
    assert {a["args"] for a in F.plan("eq", ell=G.EQ_RING_ELL, inline_args=1)["parts"]} == {"inline"}
    import inspect
    assert "ctx_staged" in inspect.signature(G.test_eq_ring_wrapped_without_a_wait).parameters
    assert [F.plan("eq", ell=e)["ok"] for e in G.EQ_REFUSED] == [False] * 3 and F.EQ_MAX_ELL + 1 in G.EQ_REFUSED and 0 in G.EQ_REFUSED
    assert F.plan("eq", ell=F.EQ_MAX_ELL)["ok"]
    # --- the result area
    cap = (K["HMAP_SIZE"] - K["HMAP_IN"]) // 32
    assert max(G.HEADS_CASES) == cap and F.plan("heads", ntabs=cap)["ok"] and not F.plan("heads", ntabs=cap + 1)["ok"]
    assert F.plan("heads", ntabs=4, count=256)["ok"] and not F.plan("heads", ntabs=5, count=205)["ok"]
    assert {256, 257} <= set(G.HEADS_CASES)      # one block of k_bind_top_list against two


# ------------------------------------------------------------------ no compared sum is blind to a boundary index
def test_no_compared_sum_is_blind_to_a_boundary_index():
    """For every sum-check, dot and evaluate call of the GPU module: the term that index 0, the last index of the first block, the first of
    the second, the last index and the first index of a second grid-stride pass contributes to each compared sum is not zero (the single
    term, not the sum). A zero here is mended in the case list (another table offset or challenge), not excused - except for the halves
    that a coordinate of 0 or one removes from the "cycle" vectors of evaluate, as the case list says."""
    zero = []
    for key, T, r in _chain_calls():
        call, kind, length, _ = key
        for i in F.boundary_indices(_plan(key)):
            for t in F.POINTS[kind]:
                term = F.sc_term(kind, T, i, t) if call == "sc_eval" else F.sc_bound_term(kind, T, r, i, t)
                if term == 0:
                    zero.append((key, i, t))
    for key, spec, r in _round_calls():
        call, kind, length, _ = key
        T = G.case_tables(*spec)
        for i in F.boundary_indices(_plan(key)):
            for t in F.POINTS[kind]:
                term = F.sc_term(kind, T, i, t) if call == "sc_eval" else F.sc_bound_term(kind, T, r, i, t)
                if term == 0:
                    zero.append((key, i, t))
    ao, bo = G.DOT_OFF
    for n in G.DOT_N:
        A, B = F.edge_table("a", n + ao, G.DOT_BASE)[ao:], F.edge_table("c", n + bo, G.DOT_BASE + 1)[bo:]
        zero += [("dot", n, i) for i in F.boundary_indices(F.plan("dot", n)) if F.dot_term(A, B, i) == 0]
    for ell in G.EVAL_ELLS:
        p = F.plan("evaluate", ell=ell)
        Z = F.edge_table("a" if ell % 2 else "c", 1 << ell, G.EVAL_BASE + ell)
        for vec in G.EVAL_VECTORS:
            r = G.challenge_vector(vec, ell)
            for th in F.boundary_indices(p):
                for k in range(1 << p["topb"]):      # the entries thread th adds up: k 2^(ell - topb) + th
                    i = (k << (ell - p["topb"])) + th
                    removed = any((rk == 0 and (i >> (ell - 1 - b)) & 1) or (rk == F.ONE and not (i >> (ell - 1 - b)) & 1) for b, rk in enumerate(r))
                    term = S.mm(Z[i], F.chi_at(r, i))
                    assert not (removed and term), "a removed entry must contribute nothing"
                    assert vec == "cycle" or not removed
                    if term == 0 and not removed:
                        zero.append(("evaluate", ell, vec, i))
            assert vec != "cycle" or ell < 2 or F.evaluate(Z, r) != 0      # what is left of the cycle cases is still a non-zero value
    assert zero == []


def test_the_gpu_case_lists_keep_the_cases_they_were_given():
    """the cases the module was specified with, by name: none is dropped or swapped (others may join them)"""
    assert set(G.EQ_ELLS) >= set(range(1, 14)) | {14, 15, 17} and set(G.EQ_VECTORS) == {"zero", "one", "minus", "cycle", "random"}
    assert (G.EQ_RING_ELL, G.EQ_RING_CALLS) == (14, 10) and {0, 33, 41} <= set(G.EQ_REFUSED)
    assert {(k, n, l) for k, n, l, _, _ in G.CHAIN_CASES} >= {(k, 1 << 16, l) for k in (0, 2) for l in "ac"} | {(1, 1 << 12, "a")}
    rc = {(c, k, n) for c, k, n, *_ in G.ROUND_CASES}
    assert rc >= {("sc_eval", k, n) for k in (0, 1, 2) for n in (1 << 17, 1 << 18)} | {("sc_bind_eval", k, n) for k in (0, 1, 2) for n in (1 << 18, 1 << 19)}
    assert rc >= {("sc_eval", 0, 1 << 20), ("sc_bind_eval", 0, 1 << 21)}
    assert {(k, n // 4, rows) for k, n, rows, *_ in G.COMMIT_CASES} >= {(2, 8192, 8), (1, 1, 1), (0, 1 << 17, 1)}
    assert set(G.DOT_N) >= {1, 255, 256, 257, 245760, 245761, 262144, 262145}
    assert set(G.EVAL_ELLS) >= {1, 2, 3, 4, 5, 12, 13} and "cycle" in G.EVAL_VECTORS
    assert set(G.VECMAT_CASES) >= {(1, 1), (1, 65), (3, 63), (4, 64), (16, 64), (17, 33), (128, 32), (129, 31), (64, 65536)}
    assert set(G.BIND_TOP_CASES) >= {(nt, n) for nt in (1, 4, 5, 9) for n in (2, 1024)}
    assert set(G.HEADS_CASES) >= {1, 256, 257, 1024}
    assert set(G.SPLIT_LENS) >= {1, 257, 1024} and set(G.SPLIT_W) >= {1, 3, 4, "len"}
    for kind, len0, layout, base, cstart in G.CHAIN_CASES:      # every chain meets every challenge of the cycle
        assert {r for r, _, _ in G.chain_model(kind, len0, layout, base, cstart)[1:]} == set(F.edge_challenges(len0 + kind))
