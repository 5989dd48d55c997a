"""CPU checks of tests/spark_reference.py, the Python-integer models that tests/test_gpu_spark_edges.py compares the SPARK kernels with:
the models against the oracle on edge tables, the exact identities the device relies on (the two-rounds cubic, the eq table as a factor,
the weighted form), and the coverage of the GPU module's case lists: together they must reach every boundary of the library's dispatch
arithmetic, so a changed constant that slides a case off its boundary fails here, without a GPU."""
import ctypes, random
import pytest
from tests import field_vectors as V
from tests import spark_reference as S
from tests import test_gpu_spark_edges as G      # the case lists only: that module imports the binding inside its tests
from tests.helpers import Q, R, sz, u64x4

EDGE_R = [0, R % Q, Q - 1]


def _arr(vals):
    return (ctypes.c_uint64 * (4 * len(vals))).from_buffer_copy(V.pack(vals))


def _ints(arr, n=None):
    raw = bytes(arr)
    n = len(raw) // 32 if n is None else n
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


def _challenges(seed):
    return EDGE_R + [random.Random(seed).randrange(Q)]


def test_the_edge_pool_is_what_the_models_are_written_for():
    pool = S.edge_pool()
    assert len(pool) == 2968 and len(set(pool)) == 1197 and pool.count(0) == 46 and max(pool) < Q
    from tests import test_gpu_field_lanes as F
    for layout in "ac":
        assert S.edge_table(layout, 300, 5) == F._table(layout, 300, 5)      # one indexing in both modules
    t = S.nonzero_edge_table("a", 2968, 0)
    assert 0 not in t and t.count(Q - 1) >= 46 and [x for x in t if x != Q - 1] == [x for x in pool if x and x != Q - 1]
    assert S.edge_challenges(3)[:3] == EDGE_R and S.edge_challenges(3)[3] not in EDGE_R


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("n", [2, 64, 8192])
def test_models_match_the_oracle_on_edge_tables(orc, n, layout):
    A, B, C = (S.edge_table(layout, n, k) for k in (0, 1, 2))
    w = (ctypes.c_uint64 * 12)()
    orc.orc_sumcheck_eval(ctypes.c_int(1), _arr(A), _arr(B), _arr(C), None, sz(n), w)
    assert S.cubic_evals(A, B, C) == _ints(w, 3)
    e4 = S.cubic_evals4(A, B, C)
    assert [e4[0], e4[2], e4[3]] == _ints(w, 3)
    o = u64x4(); orc.orc_dot(_arr(A), _arr(B), sz(n), o)
    assert S.dot_many(A, [B]) == _ints(o)
    for r in _challenges(n):
        for T in (A, C):
            z = _arr(T)
            orc.orc_bound_top(z, sz(n), _arr([r]))
            assert S.bind(T, r) == _ints(z, n // 2), (hex(r), layout, n)
    assert (e4[0] + e4[1]) % Q == S.dot3(A, B, C)      # the t = 1 value: e(0) + e(1) is the sum over the whole cube


@pytest.mark.parametrize("layout", ["a", "c"])
@pytest.mark.parametrize("n", [4, 8, 256])
def test_the_two_rounds_cubic_predicts_the_round_after_the_bind(n, layout):
    """predict(bind2_coeffs(T), r) == cubic_evals(bind(T, r)): what lets one trip advance two rounds (comment above k_cubic_bind2_eval)"""
    A, B, C = (S.edge_table(layout, n, k) for k in (3, 4, 5))
    A = A[:n // 2] * 2      # x1 - x0 = 0 in every pair of one table
    co = S.bind2_coeffs(A, B, C)
    for r in _challenges(n + 1):
        assert S.predict(co, r) == S.cubic_evals(S.bind(A, r), S.bind(B, r), S.bind(C, r)), (hex(r), n, layout)


@pytest.mark.parametrize("rho_kind", ["random", "edge"])
def test_the_eq_table_as_a_factor(rho_kind):
    """kappa(t) q(t) equals the generic evaluation when C is a real eq table (comment above quad_point_eq), cleared of its division:
    first round (1 - rho_0) E(t) = eq(t, rho_0) q(t); after a bind at r, (1 - rho_0)(1 - rho_1) E'(t) = eq(r, rho_0) eq(t, rho_1) q'(t), with q, q' over
    the leading entries of the ORIGINAL table"""
    ell = 6
    rng = random.Random(66)
    rho = [rng.randrange(Q) for _ in range(ell)]
    if rho_kind == "edge":
        rho[0], rho[1], rho[2] = Q - 1, 0, S.edge_pool()[17]
    C = S.eq_table(rho)
    A, B = S.edge_table("a", 1 << ell, 6), S.edge_table("c", 1 << ell, 7)
    om0, om1 = (S.ONE - rho[0]) % Q, (S.ONE - rho[1]) % Q
    E = S.cubic_evals4(A, B, C)
    assert S.quad_eq(A, B, C) == [S.quad_eq_at(A, B, C, 0), S.quad_eq_at(A, B, C, 2)]
    for t in range(4):
        assert S.mm(om0, E[t]) == S.mm(S.eq_at(t, rho[0]), S.quad_eq_at(A, B, C, t)), t
    for r in _challenges(7):
        A1, B1, C1 = S.bind(A, r), S.bind(B, r), S.bind(C, r)
        E1 = S.cubic_evals4(A1, B1, C1)
        eq_r = (S.mm((S.ONE - r) % Q, om0) + S.mm(r, rho[0])) % Q
        for t in range(4):
            assert S.mm(S.mm(om0, om1), E1[t]) == S.mm(S.mm(eq_r, S.eq_at(t, rho[1])), S.quad_eq_at(A1, B1, C, t)), (hex(r), t)
        k = S.mm(eq_r, pow(om0 * S.RINV % Q, Q - 2, Q) * R % Q)      # K_1 = eq(r, rho_0) / (1 - rho_0): K_1 C_original[0..len) IS the bound table
        if om0:
            assert [S.mm(k, x) for x in C[:len(C1)]] == C1


def test_the_weighted_form_is_the_weighted_sum_of_the_instances():
    n, ninst = 64, 6
    T = [[S.edge_table("a", n, 3 * k + j) for j in range(3)] for k in range(ninst)]
    cyc = S.edge_challenges(9)
    w = [cyc[(k + 1) % 4] for k in range(ninst)]
    per_e = [S.cubic_evals(*t) for t in T]
    per_c = [S.bind2_coeffs(*t) for t in T]
    assert S.weighted(per_e, w) == [sum(S.mm(w[k], per_e[k][j]) for k in range(ninst)) % Q for j in range(3)]      # as the device adds it up
    assert S.weighted(per_c, w) == [sum(S.mm(w[k], per_c[k][j]) for k in range(ninst)) % Q for j in range(12)]
    for r in cyc:      # the cubic is linear in the coefficients: the weighted coefficients predict the weighted mid-round
        mid = [S.cubic_evals(*[S.bind(x, r) for x in t]) for t in T]
        assert S.predict(S.weighted(per_c, w), r) == S.weighted(mid, w)
        assert [x for k in range(ninst) for x in S.predict(per_c[k], r)] == [x for m in mid for x in m]


def test_hash_and_product_models_on_small_inputs():
    one = S.ONE
    two, three, five = 2 * one % Q, 3 * one % Q, 5 * one % Q
    # (ts + 1) r^2 + val r + addr - gamma with r = 2, val = 3, ts = 5, addr = index 7, gamma = 1: 6 * 4 + 6 + 7 - 1 = 36
    assert S.hash_leaf(S.index_residue(7), three, five, 1, two, one) == 36 * one % Q
    assert S.hash_leaf(0, three, 0, 0, two, 0) == 6 * one % Q
    lv = [S.index_residue(i) for i in (2, 3, 5, 7, 11, 13, 17, 19)]
    st = S.product_layers(lv)
    assert len(st) == 14 and st[8:12] == [S.index_residue(x) for x in (22, 39, 85, 133)] and st[12:] == [S.index_residue(22 * 85), S.index_residue(39 * 133)]
    assert S.product_layers(lv[:2]) == lv[:2]
    assert S.dot3(lv[:3], lv[3:6], lv[5:8]) == S.index_residue(2 * 7 * 13 + 3 * 11 * 17 + 5 * 13 * 19)


# ------------------------------------------------------------------ the GPU module's case lists against the dispatch arithmetic
def test_the_named_constants_are_read_from_the_source():
    K = S.constants()
    assert set(K) == {"HOST_SUM_BYTES", "TAIL_OFF", "TAIL_MAX_INST"} and all(isinstance(v, int) and v > 0 for v in K.values())
    # the 18 sums of the most instances whose tables are handed over end below the tables in the same result page
    assert 32 * 18 * K["TAIL_MAX_INST"] <= K["TAIL_OFF"] < 32 * 18 * (K["TAIL_MAX_INST"] + 1)
    with pytest.raises(AssertionError, match="no longer defined"):
        S._constant("spark.hip", "A_CONSTANT_THAT_IS_NOT_THERE")


def test_the_dispatch_of_a_batched_round_is_written_once():
    """the tiny threshold, the inline-arguments test, the scan for the first user of a distinct C and the host-side sum of the per-block partials
    each occur exactly once in spark.hip - the text itself, and its distinctive fragment under any variable names"""
    counts = S.source_text_counts()
    assert len(S.SOURCE_TEXT_ONCE) == 4 and len(counts) == 8 and "<= 8192" in S.SOURCE_TEXT_ONCE[0] and "ninst <= 24" in S.SOURCE_TEXT_ONCE[1]
    assert all(f in t for f, t in zip(S.SOURCE_FRAGMENT_ONCE, S.SOURCE_TEXT_ONCE))
    assert counts == {t: 1 for t in counts}, {t: n for t, n in counts.items() if n != 1}


def test_the_record_shapes_sit_on_each_side_of_each_branch():
    """the shapes of test_records_and_round_trips_of_every_batched_round_call come from the case lists, and plan() says which branch each takes"""
    assert set(G.RECORD_CHAIN) <= {(n, i) for n, i, _, _ in G.CHAIN_CASES} and set(G.RECORD_EQ) <= set(G.EQ_CASES)
    assert set(G.RECORD_TWO) <= {(e, i) for e, i, _, _ in G.TWO_ROUND_CASES}
    one = {(c, n, i): S.plan(c, n, i) for n, i in G.RECORD_CHAIN for c in ("eval", "bind_eval")}
    key = lambda p: (p["form"], p["sums"], p["args"])
    assert [key(one["eval", n, i]) for n, i in G.RECORD_CHAIN] == [("tiny", "host", "inline"), ("tiny", "host", "staged"), ("tiny", "kernel", "staged"),
                                                                    ("streaming", "kernel", "inline")]
    assert key(one["bind_eval", 1 << 15, 5]) == ("tiny", "kernel", "inline") and key(one["bind_eval", 256, 64]) == ("tiny", "host", "staged")
    assert [S.plan("eq", G.EQ_LEN, ninst=i, neq=e)["generic_launch"] for e, i in G.RECORD_EQ] == [False, True]
    two = {(e, i, nb, wt): S.plan("bind2", 1 << e, i, nb, wt) for e, i in G.RECORD_TWO for nb in (0, 2) for wt in (False, True)}
    assert two[3, 21, 2, True]["tail"] and two[3, 21, 0, True]["tail"] and not two[3, 22, 2, True]["tail"] and not two[3, 21, 2, False]["tail"]
    assert all(p["sums"] == "host" for (e, _, _, _), p in two.items() if e == 3) and all(p["sums"] == "kernel" for (e, _, _, _), p in two.items() if e != 3)
    assert {p["args"] for (e, i, _, _), p in two.items() if i <= 22} == {"inline"} and {p["args"] for (e, i, _, _), p in two.items() if i >= 25} == {"staged"}


def _one_round_calls(cases):
    for len0, ninst, _, _ in cases:
        ln = len0
        while ln >= 2:
            yield ("eval", ln, ninst), S.plan("eval", ln, ninst)
            if ln >= 4:
                yield ("bind_eval", ln, ninst), S.plan("bind_eval", ln, ninst)
            ln //= 2


def _two_round_trips(cases):
    """the trips test_two_round_trips_on_edge_values makes: (length before the binds, nbind, ninst, tables asked for)"""
    for ell, ninst, _, _ in cases:
        n = 1 << ell
        yield n, 0, ninst, False
        if n <= 16:
            yield n, 0, ninst, True
        ln = n
        while ln >= 2:
            nb = 2 if ln >= 4 else 1
            yield ln, nb, ninst, (ln >> nb) <= 16
            ln >>= nb


def test_the_gpu_case_list_reaches_every_dispatch_boundary():
    K = S.constants()
    limit = K["HOST_SUM_BYTES"] // 96      # blocks x instances the host still adds up (320)
    one = dict(_one_round_calls(G.CHAIN_CASES))
    # tiny / streaming
    assert {p["form"] for (c, _, _), p in one.items() if c == "eval"} == {"tiny", "streaming"}
    assert "tiny" in {p["form"] for (c, _, _), p in one.items() if c == "bind_eval"}
    for call in ("eval", "bind_eval"):
        mine = [p for (c, _, _), p in one.items() if c == call]
        # host-summed: one block; blocks x instances exactly at the limit; the first reachable product above it (block counts are powers of two)
        assert any(p["nblk"] == 1 and p["sums"] == "host" for p in mine), call
        assert any(p["nblk"] > 1 and p["product"] == limit and p["sums"] == "host" for p in mine), call
        first_above = min(b * i for b in (1 << k for k in range(1, 14)) for i in range(1, S.MAX_INST + 1) if b * i > limit)
        assert any(p["product"] == first_above and p["sums"] == "kernel" for p in mine), (call, first_above)
        assert any(p["form"] == "tiny" and p["sums"] == "kernel" for p in mine), call
        # arguments
        for ninst, args in ((S.INLINE_MAX_INST, "inline"), (S.INLINE_MAX_INST + 1, "staged"), (S.MAX_INST, "staged")):
            assert any(i == ninst and p["args"] == args for (c, _, i), p in one.items() if c == call), (call, ninst)
        assert any(i == 1 for (c, _, i), _ in one.items() if c == call)
    assert any(p["args"] == "staged" and p["sums"] == "host" for p in one.values()) and any(p["args"] == "staged" and p["sums"] == "kernel" for p in one.values())
    # the two-rounds family
    trips = [(t, S.plan("bind2", t[0], t[2], t[1], t[3])) for t in _two_round_trips(G.TWO_ROUND_CASES)]
    assert {p["sums"] for _, p in trips} == {"host", "kernel"}
    assert any(t[2] == K["TAIL_MAX_INST"] and p["tail"] for t, p in trips)
    assert any(t[2] == K["TAIL_MAX_INST"] + 1 and t[3] and 2 <= p["n2"] <= 8 and not p["tail"] for t, p in trips)
    for n2 in (2, 4, 8):
        assert any(t[2] == K["TAIL_MAX_INST"] and p["n2"] == n2 and p["tail"] for t, p in trips), n2
    assert {1, 2, 4, 8, 16} <= {p["n2"] for _, p in trips}
    assert any(t[2] == S.INLINE_MAX_INST and p["args"] == "inline" for t, p in trips)
    assert any(t[2] == S.INLINE_MAX_INST + 1 and p["args"] == "staged" and p["sums"] == "kernel" for t, p in trips)
    assert any(t[2] == S.INLINE_MAX_INST + 1 and p["args"] == "staged" and p["sums"] == "host" for t, p in trips)
    assert any(t[2] == S.MAX_INST for t, _ in trips) and any(t[2] == 1 for t, _ in trips)
    assert any(t[3] and p["n2"] == 16 and not p["tail"] for t, p in trips)      # too long to hand over
    # product trees
    trees = [(c, S.plan("tree", c[0], count=c[1])) for c in G.TREE_CASES]
    kinds = [[k for k, _ in p["launches"]] for _, p in trees]
    assert [] in kinds and ["tail"] in kinds and ["one", "tail"] in kinds and ["two", "tail"] in kinds and ["two", "one", "tail"] in kinds
    assert {1, 2, 3} <= {p["chunks"] for _, p in trees}
    assert any(c[1] == S.TREE_CHUNK and p["chunks"] == 1 for c, p in trees) and any(c[1] == S.TREE_CHUNK + 1 and p["chunks"] == 2 for c, p in trees)
    assert any(p["launches"] == [("tail", S.TREE_TAIL_MAX)] for _, p in trees) and any(p["launches"][0] == ("two", S.TREE_TWO_MIN) for _, p in trees if p["launches"])
    # the eq-factored form
    eqs = [S.plan("eq", G.EQ_LEN, ninst=ni, neq=ne) for ne, ni in G.EQ_CASES]
    assert all(p["ok"] for p in eqs) and {p["generic_launch"] for p in eqs} == {False, True}
    assert G.EQ_LEN == S.EQ_MIN_LEN and not S.plan("eq", G.EQ_LEN // 2, ninst=1, neq=1)["ok"]
    assert any(ni == S.EQ_MAX_INST and ne == ni for ne, ni in G.EQ_CASES) and any(ni == S.EQ_MAX_INST and ne < ni for ne, ni in G.EQ_CASES)
    assert not S.plan("eq", G.EQ_LEN, ninst=S.EQ_MAX_INST + 1, neq=1)["ok"]


def test_the_gpu_case_list_keeps_the_cases_it_was_given():
    """the cases the module was specified with, by name: none is dropped or swapped (others may join them)"""
    chain = {(2, 1), (4, 1), (128, 3), (256, 64), (1024, 25), (1024, 64)} | {(1 << 15, 5)}
    assert chain <= {(n, i) for n, i, _, _ in G.CHAIN_CASES}
    assert {(1 << 15, 5, 3, "a"), (1 << 15, 5, 3, "c"), (128, 3, 3, "a"), (256, 64, 63, "a")} <= set(G.CHAIN_CASES)
    two = {(e, 1) for e in (1, 2, 3, 4, 5)} | {(e, i) for e in (3, 4, 5) for i in (21, 22)} | {(6, 25), (9, 25), (4, 64), (13, 5)}
    assert two <= {(e, i) for e, i, _, _ in G.TWO_ROUND_CASES}
    for e in (1, 2, 3, 4, 5):
        assert {w is None for ee, i, w, _ in G.TWO_ROUND_CASES if (ee, i) == (e, 1)} == {True, False}
    assert all(w is not None for e, i, w, _ in G.TWO_ROUND_CASES if i in (21, 22, 25) or e == 13)
    assert {(13, 5, "a"), (13, 5, "c")} <= {(e, i, l) for e, i, _, l in G.TWO_ROUND_CASES}
    assert set(G.EQ_CASES) >= {(1, 1), (24, 24), (3, 24)} and G.EQ_LEN == 65536
    assert set(G.TREE_CASES) >= {(2, 3), (2048, 16), (2048, 17), (4096, 33), (8192, 2), (16384, 2)} and set(G.TREE_SINGLE) >= {2, 4, 2048, 4096}
    assert {(nt, n) for nt, n, _ in G.DOT_MANY_CASES} >= {(nt, n) for nt in (1, 64) for n in (1, 255, 256, 257, 3000)}
    assert any(kind == "minus_one" for _, _, kind in G.DOT_MANY_CASES)
