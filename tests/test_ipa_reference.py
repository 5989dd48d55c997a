"""CPU checks of tests/ipa_reference.py and of the case lists of tests/test_gpu_ipa_edges.py: the flat form of the inner-product argument equals
the reference's folded-generator algorithm byte for byte (which licenses it for the openings above 4096), the digit model satisfies the
recoding identity on the digit pool of every geometry the GPU list uses, the thresholds the plan restates are still in ipa.hip / commit.hip /
tree.hpp, and the GPU case lists reach every boundary of the host state machine on both sides."""
import random
import pytest
from tests import ipa_reference as I
from tests import test_gpu_ipa_edges as G      # the case lists and the pure-Python case builders: the binding is imported inside its tests
from tests.helpers import Q, gens_bytes


@pytest.fixture(scope="module")
def points(orc):
    comp = gens_bytes(orc, 71, b"gens_ipa_reference")
    return [comp[32 * i:32 * i + 32] for i in range(72)]


def _rounds(ev):
    return [e[1] for e in ev if e[0] == "round"]


def _trace(n0, name, steps, order=G.ORDERS["host_first"], a_last_zero=False, **o):
    return I.trace(n0, G.geom_of(name).nwin, steps, G.opts_for(name, **o), order, a_last_zero)


# ------------------------------------------------------------------ the two forms of the argument
@pytest.mark.parametrize("n0", [1, 2, 4, 8, 64])
def test_flat_rows_equal_the_folded_generator_algorithm(orc, points, n0):
    rng = random.Random(n0)
    cases = [("edge", I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng), {}),
             ("q is h", I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng), dict(q_idx=n0 + 3, h_idx=n0 + 3)),
             ("offset", I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng), dict(g_off=6, q_idx=2, h_idx=0))]
    if n0 >= 4:
        sc = I.make_script(n0, rng)
        tgt = [0] + [rng.randrange(1, Q) for _ in range(n0 // 2 - 1)]
        a = I.a_reaching(n0, sc, 1, tgt, rng)
        assert a[0] and a[n0 // 2] and (a[0] * sc["steps"][1][1] + sc["steps"][1][2] * a[n0 // 2]) % Q == 0      # zero only after the fold
        cases.append(("folded zero", a, I.edge_vector(n0, rng), sc, {}))
        cases.append(("two folds", I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng, double_fold_at=1), {}))
    for what, a, b, sc, kw in cases:
        fo, fl = I.folded_reference(orc, points, a, b, sc, **kw), I.flat_reference(orc, points, a, b, sc, **kw)
        assert fo == fl, (n0, what)
        assert len(fo["L"]) == len([s for s in sc["steps"] if s[0] == "round"])
        part = I.flat_reference(orc, points, a, b, sc, max_rounds=1, threads=2, **kw)
        assert part == {"L": fo["L"][:1], "R": fo["R"][:1]}, (n0, what)


def test_the_model_states_the_identity_of_the_header():
    """include/spartan_hip.h: the folded generator G'[i] is sum_p s[p] G[p n_cur + i] — here with integers for points (G[j] = a random residue)"""
    rng = random.Random(3)
    n0 = 16
    Gv = [rng.randrange(Q) for _ in range(n0)]
    m = I.IpaModel([1] * n0, [1] * n0)
    cur = list(Gv)
    for _ in range(4):
        u = rng.randrange(1, Q)
        ui = I.INV(u)
        h = len(cur) // 2
        cur = [(ui * cur[i] + u * cur[h + i]) % Q for i in range(h)]      # bullet.rs:108
        m.fold(u, ui)
        assert cur == [sum(m.s[p] * Gv[p * m.n_cur + i] for p in range(n0 // m.n_cur)) % Q for i in range(m.n_cur)]
    assert [s for s, _ in m.ghat_row()] == m.s and [j for _, j in m.ghat_row()] == list(range(n0))


# ------------------------------------------------------------------ digits
def _geoms():
    return sorted({G.SETS[n][2:] for n in G.SETS})


@pytest.mark.parametrize("wbits,windows", _geoms())
def test_digit_model_on_the_digit_pool(wbits, windows):
    ge = I.Geom(wbits=wbits, windows=windows)
    assert sum(ge.width(w) for w in range(ge.nwin)) >= 254 and ge.bitpos(ge.nwin - 1) + ge.width(ge.nwin - 1) >= 254
    assert all(ge.bitpos(w + 1) == ge.bitpos(w) + ge.width(w) for w in range(ge.nwin - 1))
    pool = I.digit_pool(ge)
    rng = random.Random(wbits * 100 + windows)
    for s in pool + I.edge_pool() + [rng.randrange(Q) for _ in range(50)]:
        d = ge.digits(s)
        assert sum(dw << ge.bitpos(w) for w, dw in enumerate(d)) == s      # the oracle-free identity
        assert all(-ge.half(w) <= dw < ge.half(w) for w, dw in enumerate(d))
    # what the pool is for: in every window a field exactly at the window's tent (digit -tent, carry out) and one below (the largest digit),
    # in narrow and in wide windows; a carry that runs through every window; a carry that tips a window standing at tent - 1
    for w in range(ge.nwin):
        if (ge.half(w) << ge.bitpos(w)) < Q:
            assert any(ge.field(s, w) == ge.half(w) and ge.digits(s)[w] == -ge.half(w) for s in pool), w
        assert any(ge.field(s, w) == ge.half(w) - 1 and ge.digits(s)[w] == ge.half(w) - 1 for s in pool) or (ge.half(w) - 1) << ge.bitpos(w) >= Q, w
        if 0 < w and (ge.half(w) << ge.bitpos(w)) < Q:
            assert any(ge.field(s, w) == ge.half(w) - 1 and ge.digits(s)[w] == -ge.half(w) for s in pool), w
    top = 252 // ge.wbits if not ge.nwide else max(w for w in range(ge.nwin) if ge.bitpos(w) <= 252)
    d = ge.digits(2**252 - 1)
    assert d[0] == -1 and all(x == 0 for x in d[1:top]) and d[top] > 0      # one carry from window 0 to the window of bit 252
    assert (2**253 - 1) % Q in pool and 2**252 - 1 in pool
    chunks = G.digit_chunks(ge)
    assert all(len(c) == 8 for c in chunks) and {s for c in chunks for s in c} == set(pool)


def test_the_edge_pool_is_the_pool_of_the_helpers():
    from tests.helpers import rand_scalars
    pool = I.edge_pool()
    assert len(pool) == len(set(pool)) == 12 and {0, 1, Q - 1, 2**252} <= set(pool)
    assert set(rand_scalars(random.Random(1), 2000, "edge")) == set(pool)


# ------------------------------------------------------------------ the plan and the source
def test_the_thresholds_are_still_in_the_source():
    assert I.source_text_missing() == []
    K = I.constants()
    assert (K["C0_PAIRS"], K["C0_MAX_BLOCKS"], K["FUSED_MAX_N"], K["DOT_PER_BLOCK"], K["LOOKUPS_PER_BLOCK"], K["TREE_TOP"]) == (512, 16, 16384, 64, 256, 128)
    # the last fused size is the largest the first-round partial pairs and the dot-product partials both still serve
    assert K["C0_MAX_BLOCKS"] * K["C0_PAIRS"] * 2 == K["FUSED_MAX_N"]


def test_the_value_cases_hold_the_relation_their_name_says():
    for n0 in G.VALUE_N:
        lg = n0.bit_length() - 1
        for name in G.VALUE_CASES:
            a, b, sc = G.value_case(n0, name)
            res, _ = I.run_model(a, b, sc)
            rounds = res["rounds"]
            zeros = lambda k: sum(1 for s, _ in rounds[k][2][:-2] + rounds[k][3][:-2] if s == 0)
            if name == "folded_zero_round2":
                assert all(a) and zeros(0) == 0 and zeros(1) >= 2      # zero only after the fold: no entry of a itself is zero
            elif name in ("folded_zero_last", "a_last0_zero", "a_last1_zero"):
                last = rounds[-1][4]["a"]
                assert [x == 0 for x in last] == {"folded_zero_last": [True, True], "a_last0_zero": [True, False], "a_last1_zero": [False, True]}[name]
                assert all(a) and all(zeros(k) == 0 for k in range(lg - 1)) and zeros(lg - 1) > 0
            elif name == "cL_zero":
                assert rounds[0][0] == 0 and rounds[0][1] != 0 and all(b)
            elif name == "q_scale_zero":
                assert all(r[2][-2][0] == 0 and r[3][-2][0] == 0 and r[0] and r[1] for r in rounds)
            elif name == "zero_blinds":
                assert all(r[2][-1][0] == 0 and r[3][-1][0] == 0 for r in rounds)
            elif name in ("d_zero", "d_r_zero"):
                assert all(s == 0 for s, _ in res["delta_row"][:-1]) and (res["delta_row"][-1][0] == 0) == (name == "d_r_zero")
            elif name in ("u_one", "u_minus_one"):
                want = 1 if name == "u_one" else Q - 1
                assert all(c == (want, want) for c in I.challenges(sc))
            elif name == "b_zero":
                assert all(r[0] == 0 and r[1] == 0 for r in rounds) and res["b_hat"] == 0
            elif name == "a_one_hot":
                assert sum(1 for x in a if x) == 1 and res["a_hat"] != 0


def test_the_gpu_case_lists_reach_every_boundary_of_the_state_machine():
    K = I.constants()
    # ---- sizes: every path the state machine takes by size, on both trees
    first, all_rounds = {}, {}
    for n0 in G.SIZE_CASES:
        for tree in G.TREES:
            name = G.set_for(n0, tree)
            ev = _trace(n0, name, G.size_case(n0, tree)[2]["steps"])
            first[n0, tree], all_rounds[n0, tree] = ev, _rounds(ev)
            assert all(p["tree"] == ("dedicated" if tree == "derived" else "unified") and p["fusable"] for p in all_rounds[n0, tree])
            assert len(all_rounds[n0, tree]) == n0.bit_length() - 1
    for tree in G.TREES:
        r = all_rounds
        assert first[1, tree][0][1]["n1_arm"] and not first[1, tree][0][1]["want_c0"] and r[1, tree] == []      # n0 = 1: no round,
        assert first[1, tree][1] == ("finish_commit", "device", 0)                                              # and no host finish
        p = r[2, tree][0]      # n0 = 2: the first round is the last; two of a quad's four lanes are live
        assert p["last"] and p["fold"] == 0 and p["qlen"] == 1 and p["dot_lanes_live"] == 2 and p["leaves_fin"] and not p["leaves_dots"] and p["nd"] == 1
        assert first[2, tree][-3] == ("finish_commit", "host", 1)
        p = r[4, tree]         # n0 = 4: the second round reads the dots and is the last
        assert [q["fold"] for q in p] == [0, 1] and p[0]["leaves_dots"] and p[1]["last"] and p[0]["dot_lanes_live"] == 4
        assert [q["n_cur"] for q in r[8, tree]] == [8, 4, 2]
        # one | two blocks of quarter dot products, one | two blocks of k_ipa_init: on both sides, in the FIRST round (what the size decides)
        assert (r[256, tree][0]["qlen"], r[256, tree][0]["nd"], r[512, tree][0]["nd"]) == (K["DOT_PER_BLOCK"], 1, 2)
        assert (first[1024, tree][0][1]["nblk0"], first[2048, tree][0][1]["nblk0"]) == (1, 2) and 1024 // 2 == K["C0_PAIRS"]
    # ---- the row reducer: exactly 256 partial sums, more than 256 (the strided loop), and fewer everywhere else
    red = {}
    for name, ded in G.REDUCER_CASES:
        ev = _trace(4096, name, G.size_case(4096, name)[2]["steps"], dedicated_uploaded=ded)
        red[name, ded] = _rounds(ev)[0]
        assert all(p["fusable"] and p["tree"] == ("dedicated" if ded else "unified") for p in _rounds(ev))
    for ded in (0, 1):
        assert red["u4098w8", ded]["nblk"] == K["REDUCE_STRIDE"] == red["u4098w8", ded]["reduce_count"] and not red["u4098w8", ded]["reduce_strided"]
        assert red["u4098w5", ded]["nblk"] == 408 and red["u4098w5", ded]["reduce_strided"] and red["u4098w5", ded]["reduce_count"] == 256
    assert max(p["nblk"] for rr in all_rounds.values() for p in rr) < K["REDUCE_STRIDE"]
    # ---- large: 16384 is the last fused size (16 blocks of k_ipa_init, 64 dot blocks); 32768 never fuses
    large = {}
    for n0, rounds in G.LARGE_CASES:
        ev = _trace(n0, "d32770", G.large_case(n0)[2]["steps"])
        large[n0] = (ev[0][1], _rounds(ev))
    assert set(large) == {8192, 16384, 32768}
    assert large[8192][0]["nblk0"] == 8 and all(p["fusable"] and p["reduce_strided"] for p in large[8192][1][:1])
    b, r = large[16384]
    assert b["nblk0"] == K["C0_MAX_BLOCKS"] and b["want_c0"] and r[0]["n_cur"] == K["FUSED_MAX_N"] and r[0]["nd"] == 64 and all(p["fusable"] for p in r)
    assert 1024 + (r[0]["nd"] * 8 + 4) * 32 <= 30720      # the dot-product partials and a', b' fit the result page (ipa_round_launch)
    b, r = large[32768]
    assert b["nblk0"] == 2 * K["C0_MAX_BLOCKS"] and not b["want_c0"] and not any(p["fusable"] for p in r)
    assert [p["fold"] for p in r] == [0] + [1] * 14 and all(p["prepare_grid"] == 32768 // K["PREP_PER_BLOCK"] + 1 for p in r)
    # ---- the last block's tree: partly live blocks, every top level, a count that is exactly a power of two, a full block
    lasts = {(p["last_count"], p["last_top"]) for rr in all_rounds.values() for p in rr}
    for w, nw in G.DIGIT_GEOMS:
        for tree in G.TREES:
            name = "g%s_%d_%d" % (tree[0], w, nw)
            ev = _trace(8, name, I.make_script(8, random.Random(1))["steps"])
            lasts |= {(p["last_count"], p["last_top"]) for p in _rounds(ev)}
            assert all(p["tree"] == ("dedicated" if tree == "derived" else "unified") for p in _rounds(ev))
    assert {t for _, t in lasts} == {16, 32, 64, 128}
    assert {(17, 16), (34, 32), (68, 64), (128, 64), (204, 128), (256, 128)} <= lasts      # 128 = 4 x 32 windows: the level above would add nothing
    # ---- values: fused and unfused; a zero in the last pair sends sp_ipa_finish_commit to the device with the fold still pending
    for n0 in G.VALUE_N:
        for name in G.VALUE_CASES:
            a, bb, sc = G.value_case(n0, name)
            zero_last = 0 in I.run_model(a, bb, sc)[0]["rounds"][-1][4]["a"]
            assert zero_last == (name in ("folded_zero_last", "a_last0_zero", "a_last1_zero", "a_one_hot"))      # (a one-hot a stays one-hot)
            for fused in (1, 0):
                ev = _trace(n0, "d70", sc["steps"], a_last_zero=zero_last, fused=fused)
                assert all(p["fusable"] == bool(fused) for p in _rounds(ev)) and [p["fold"] for p in _rounds(ev)] == [0] + [1] * (n0.bit_length() - 2)
                assert ev[-3] == ("finish_commit", "host" if fused and not zero_last else "device", 1)
    # ---- call orders
    n0, name, extra = G.PRELAUNCH_CASE
    assert extra > 0 and all(p["fusable"] for p in _rounds(_trace(n0, name, G.order_case("prelaunch", n0)[2]["steps"])))      # the prelaunch launches
    after = set()      # what follows the flushed fold: the last round | a round with more behind it | the end of the argument
    for n0, at in G.DOUBLE_FOLD_CASES:
        ev = _trace(n0, "d70", G.order_case("double_fold", n0, double_fold_at=at)[2]["steps"])
        k = [e[0] for e in ev].index("flush_fold")
        if ev[k + 1][0] == "round":      # the dots described the vectors before the flush: this round runs on k_ipa_prepare with the second fold,
            rest = _rounds(ev[k + 1:])   # and nothing leaves dots behind after an unfused round: the rest stays there
            assert rest[0]["fold"] == 1 and not any(p["fusable"] for p in rest) and len(_rounds(ev)) == n0.bit_length() - 2
            after.add("last round" if len(rest) == 1 else "more rounds")
        else:                            # the two folds end the argument: no last round, so no host finish
            assert ev[k + 1] == ("finish_commit", "device", 1)
            after.add("end")
    assert after == {"last round", "more rounds", "end"}
    fin = {}
    for order, dev in G.FINISH_CASES:
        ev = _trace(64, "d70", G.order_case("finish", 64)[2]["steps"], order=G.ORDERS[order], finish_device=dev)
        fin[order, dev] = [e for e in ev if e[0] == "finish_commit"][0][1:]
    assert fin == {("device_first", 0): ("device", 0), ("reverse", 0): ("device", 0), ("host_first", 1): ("device", 1), ("device_first", 1): ("device", 0)}
    assert _trace(64, "d70", G.order_case("finish", 64)[2]["steps"])[-3] == ("finish_commit", "host", 1)      # (the default order: every other test)
    for n0, name in G.ENCODE_DEVICE_CASES:
        ev = _trace(n0, name, G.order_case("encode_device", n0)[2]["steps"], device_encode=1)
        assert not ev[0][1]["want_c0"] and not any(p["fusable"] for p in _rounds(ev)) and ev[-3] == ("finish_commit", "device", 1)
    # ---- positions
    npts = G.SETS["d70"][1]
    pos = {name: (g_off, n0, q, h) for name, g_off, n0, q, h in G.POSITION_CASES}
    assert any(g and q < g and h < g and q != h for g, n, q, h in pos.values())
    assert any(g + n == npts for g, n, q, h in pos.values()) and all(g + n <= npts and q < npts and h < npts for g, n, q, h in pos.values())
    assert any(q == h and q >= g + n for g, n, q, h in pos.values()) and any(q == h and q < g for g, n, q, h in pos.values())


def test_the_gpu_case_lists_keep_the_cases_they_were_given():
    assert G.SIZE_CASES == [1, 2, 4, 8, 256, 512, 1024, 2048] and G.TREES == ["derived", "uploaded"]
    assert {(G.SETS[n][2], d) for n, d in G.REDUCER_CASES} == {(8, 0), (8, 1), (5, 0), (5, 1)} and all(G.SETS[n][0] == "uploaded" for n, _ in G.REDUCER_CASES)
    assert [n for n, _ in G.LARGE_CASES] == [8192, 16384, 32768] and G.LARGE_CASES[1][1] is None and G.LARGE_CASES[2][1] in (None, 3)
    assert G.SETS["d32770"][2] == 5      # the narrowest width test_commit_rows_at_every_window_width covers
    assert G.VALUE_N == [8, 64] and len(G.VALUE_CASES) == 13
    assert set(G.DIGIT_GEOMS) == {(5, 0), (8, 0), (13, 0), (15, 0), (0, 17), (0, 18), (0, 26), (0, 32)}
    assert G.PRELAUNCH_CASE == (1024, "d2050", 37) and [n for n, _ in G.ENCODE_DEVICE_CASES] == [8, 1024]
    assert ("g_off5", 5, 64, 2, 0) in G.POSITION_CASES and any(c[1] == 6 for c in G.POSITION_CASES) and G.SETS["d70"][1] == G.SETS["u70"][1] == 70
    assert {("device_first", 0), ("reverse", 0)} <= set(G.FINISH_CASES) and any(d == 1 for _, d in G.FINISH_CASES)
