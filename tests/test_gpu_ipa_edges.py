"""The inner-product argument (spartan_amd/csrc/ipa.hip: sp_ipa_*, k_ipa_init / k_ipa_prepare / k_ipa_fold / k_ipa_finish_rows; k_ipa_round and
ipa_round_launch in commit.hip) on EDGE VALUES, at EVERY BOUNDARY OF ITS HOST STATE MACHINE, and in every call order the API allows.
tests/test_gpu_large.py holds n = 4096 on uniform random scalars; whole proofs reach the argument on random witnesses only. Here:

  sizes      n0 = 1 (no round), 2 (the first round is the last), 4, 8, 256 | 512 (one | two blocks of quarter dot products), 1024 | 2048 (one |
             two blocks of k_ipa_init), on library-derived generators (the dedicated tree, what production runs) and on uploaded ones
  reducer    n0 = 4096 at 8-bit windows (exactly 256 partial sums per row) and at 5-bit windows (408: the strided loop of the row reducer)
  large      8192, 16384 (the last size of the one-launch path: 64 dot blocks, 16 blocks of k_ipa_init) and 32768 (every round on k_ipa_prepare)
  values     a scalar that is zero only after the fold, a last pair with a zero entry (the host finish gives up), c_L = 0, Q scaled by 0,
             zero blinds, d = 0, d = r = 0 (delta is the neutral element), u = 1, u = q - 1, b = 0, a one-hot a; each fused and unfused
  digits     the digit pool of tests/ipa_reference.py (a field exactly at half a window, one below, carries through every window) as `a`, at
             uniform 5, 8, 13, 15 bits and at 17, 18, 26, 32 mixed-width windows
  orders     prelaunch + set_scale + round_lr through sp_ipa_begin_dev (table longer than n, commit_a), two folds with no round between,
             the three finishing calls in both orders and on the device, sp_ipa_free over an uncollected prelaunch, encode.device = 1
  positions  g_off = 5 and 6 (the last legal offset) in a 70-point set, Q and H below g_off, Q = H
  refusals   every argument check, each followed by correct calls on the same handle

tests/test_ipa_reference.py asserts on the CPU (through ipa_reference.plan / trace, which read the thresholds from the source) that these lists
reach every one of those boundaries on both sides. Expected bytes: the reference's own algorithm (ipa_reference.folded_reference: G folded every
round, orc_pt_msm) up to n0 = 4096, the model's flat rows above (flat_reference; the CPU module shows the two agree byte for byte). Every
comparison is exact — L and R after every round, a_hat, b_hat, g_hat, delta, commit_a — and is counted (printed when the module ends).
After an unexpected status nothing further is started (the guard of tests/test_gpu_spark_edges.py, shared).

Not reached here: openings of 65536 and more (6.8 GB of tables at the narrowest width, a reference of minutes); the re-run of a round whose
dedicated tree met an exceptional sum at any size but 16 (tests/test_gpu_large.py); the refusal inside ipa_round_launch (its dot-product
partials never outgrow the result page while n_cur <= 16384); the out-of-memory returns."""
import ctypes, hashlib, os, random
import pytest
from tests import ipa_reference as I
from tests.helpers import Q, vp, sz, gens_bytes, mont_bulk, from_mont_bulk
from tests.test_gpu_spark_edges import _DEVICE_ERROR, _ok, _refused
from tests.test_gpu_spark_edges import _nothing_after_a_device_error      # the autouse guard: a fixture of this module too

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the case lists (imported by tests/test_ipa_reference.py: no GPU needed)
# generator sets: name -> (kind, points, msm.wbits, msm.windows); a fresh label per set (a resident table set is reused whatever its width)
SETS = {"d70": ("derived", 70, 0, 17), "u70": ("uploaded", 70, 0, 17), "d2050": ("derived", 2050, 8, 0), "u2050": ("uploaded", 2050, 8, 0),
        "u4098w8": ("uploaded", 4098, 8, 0), "u4098w5": ("uploaded", 4098, 5, 0), "d32770": ("derived", 32770, 5, 0)}
DIGIT_GEOMS = [(5, 0), (8, 0), (13, 0), (15, 0), (0, 17), (0, 18), (0, 26), (0, 32)]      # (msm.wbits, msm.windows)
for _w, _n in DIGIT_GEOMS:
    for _k in ("derived", "uploaded"):
        SETS["g%s_%d_%d" % (_k[0], _w, _n)] = (_k, 10, _w, _n)
TREES = ["derived", "uploaded"]
SIZE_CASES = [1, 2, 4, 8, 256, 512, 1024, 2048]
REDUCER_CASES = [("u4098w8", 0), ("u4098w8", 1), ("u4098w5", 0), ("u4098w5", 1)]      # (set, ipa.dedicated_uploaded) at n0 = 4096
LARGE_CASES = [(8192, None), (16384, None), (32768, None)]      # (n0, rounds compared: None = the whole argument)
VALUE_N = [8, 64]
VALUE_CASES = ["folded_zero_round2", "folded_zero_last", "a_last0_zero", "a_last1_zero", "cL_zero", "q_scale_zero", "zero_blinds", "d_zero", "d_r_zero",
               "u_one", "u_minus_one", "b_zero", "a_one_hot"]
POSITION_CASES = [("g_off5", 5, 64, 2, 0), ("g_off_last", 6, 64, 3, 1), ("q_is_h", 0, 64, 69, 69), ("q_is_h_below", 5, 64, 4, 4)]      # (name, g_off, n0, q_idx, h_idx)
ORDERS = {"device_first": ("finish", "finish_commit", "commit_ghat"), "reverse": ("commit_ghat", "finish_commit", "finish"),
          "host_first": ("finish_commit", "finish", "commit_ghat")}
FINISH_CASES = [("device_first", 0), ("reverse", 0), ("host_first", 1), ("device_first", 1)]      # (order, ipa.finish_device)
DOUBLE_FOLD_CASES = [(8, 1), (64, 2), (64, 5)]      # (n0, the round after which two folds follow: the next round is the last | is not | does not exist)
ENCODE_DEVICE_CASES = [(8, "d70"), (1024, "d2050")]
PRELAUNCH_CASE = (1024, "d2050", 37)      # n0, set, entries of the device table beyond n

COUNTS = {k: 0 for k in ("sizes", "reducer", "large", "values", "digits", "orders", "positions", "refusals")}      # exact comparisons per section


def set_for(n0, tree):
    return ("d" if tree == "derived" else "u") + ("70" if n0 <= 64 else "2050")


def geom_of(name):
    _, _, w, nw = SETS[name]
    return I.Geom(wbits=w, windows=nw)


def opts_for(name, **kw):
    o = dict(I.DEFAULT_OPTS)
    o["derived"] = SETS[name][0] == "derived"
    o.update(kw)
    return o


def _seed(*parts):
    return int.from_bytes(hashlib.sha256(repr(parts).encode()).digest()[:8], "little")


def size_case(n0, tree):
    rng = random.Random(_seed("size", n0, tree))
    return I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng)


def value_case(n0, name):
    """(a, b, script) of a value case: uniform random vectors with the one relation the name says"""
    rng = random.Random(_seed("value", n0, name))
    kw = {"q_scale_zero": dict(q_scale=0), "zero_blinds": dict(zero_blinds=True), "d_zero": dict(d=0), "d_r_zero": dict(d=0, r=0),
          "u_one": dict(u=1), "u_minus_one": dict(u=Q - 1)}.get(name, {})
    sc = I.make_script(n0, rng, **kw)
    a, b = [rng.randrange(1, Q) for _ in range(n0)], [rng.randrange(1, Q) for _ in range(n0)]
    lg = n0.bit_length() - 1
    if name == "folded_zero_round2":
        h = n0 // 2
        zeros = {0, h - 1} | ({1, h // 2} if h >= 8 else set())      # in both rows of round 2, first and last lookups of a row
        tgt = [0 if i in zeros else rng.randrange(1, Q) for i in range(h)]
        a = I.a_reaching(n0, sc, 1, tgt, rng)
    elif name in ("folded_zero_last", "a_last0_zero", "a_last1_zero"):
        x = rng.randrange(1, Q)
        a = I.a_reaching(n0, sc, lg - 1, {"folded_zero_last": [0, 0], "a_last0_zero": [0, x], "a_last1_zero": [x, 0]}[name], rng)
    elif name == "cL_zero":
        b = I.b_with_cL_zero(a, b)
    elif name == "b_zero":
        b = [0] * n0
    elif name == "a_one_hot":
        a = [0] * n0
        a[n0 // 2 + 1] = rng.randrange(1, Q)
    return a, b, sc


def digit_chunks(geom):
    """the digit pool in vectors of 8 (the last one filled up from the front)"""
    pool = I.digit_pool(geom)
    pool += pool[:(-len(pool)) % 8]
    return [pool[i:i + 8] for i in range(0, len(pool), 8)]


def position_case(name, n0):
    rng = random.Random(_seed("position", name))
    return I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng)


def order_case(tag, n0, **kw):
    rng = random.Random(_seed("order", tag, n0))
    return I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng, **kw)


def large_case(n0):
    rng = random.Random(_seed("large", n0))
    return I.edge_vector(n0, rng), I.edge_vector(n0, rng), I.make_script(n0, rng)


# ------------------------------------------------------------------ the device side
@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    if _DEVICE_ERROR:
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    c = capi.Ctx(0)
    yield c
    c.close()
    print("\nexact comparisons per section: %s; total %d" % (", ".join("%s %d" % kv for kv in sorted(COUNTS.items())), sum(COUNTS.values())))


@pytest.fixture(scope="module")
def gsets(ctx, orc):
    """name -> (Gens, [compressed points]) of SETS, built on first use with the set's own window geometry"""
    from spartan_amd import capi
    from tests.test_oracle_pins import BASEPOINT
    built = {}

    def get(name):
        if name in built:
            return built[name]
        kind, n, wbits, windows = SETS[name]
        label = b"gens_ipa_edges_" + name.encode()
        ctx.set_option("msm.wbits", wbits); ctx.set_option("msm.windows", windows)      # read when a generator set is built
        try:
            if kind == "derived":
                g = capi.Gens(ctx, uniform=hashlib.shake_256(label + bytes.fromhex(BASEPOINT)).digest(64 * n))
                if n <= 4098:      # (the large set: the derivation has its own test, and the oracle would take seconds over it)
                    assert g.compressed == gens_bytes(orc, n - 1, label)
            else:
                g = capi.Gens(ctx, compressed=gens_bytes(orc, n - 1, label))
        finally:
            ctx.set_option("msm.wbits", 0); ctx.set_option("msm.windows", 0)
        ge = geom_of(name)
        assert g.windows() == ge.nwin and g.window_bits() == ge.wbits, name
        assert capi.lib.sp_gens_table_bytes(g.h) == ge.table_bytes(n), name
        built[name] = (g, [g.compressed[32 * i:32 * i + 32] for i in range(n)])
        return built[name]
    yield get
    for g, _ in built.values():
        g.free()


class _Options:
    """tier-1 options for the length of a with-block: unlocked, set, and restored in any case"""
    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, {k.replace("__", "."): v for k, v in kv.items()}

    def __enter__(self):
        self.ctx.set_option("testing.unlock", 1)
        self.old = {k: self.ctx.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)
        self.ctx.set_option("testing.unlock", 0)


def fq1(x):
    return mont_bulk([x])


def _eq(sec, got, want, what):
    hx = lambda v: v.hex() if isinstance(v, bytes) else v
    assert got == want, (what, hx(got), hx(want))
    COUNTS[sec] += 1


def drive(sec, ctx, orc, g, P, a, b, script, want, g_off=0, q_idx=None, h_idx=None, order=ORDERS["host_first"], prelaunch=False, dev_extra=None,
          max_rounds=None, after_round=None, tag=""):
    """one argument through sp_ipa_*, every output compared with `want` (folded_reference / flat_reference) right after its call.
    dev_extra: through sp_ipa_begin_dev from a device table of n + dev_extra entries, with commit_a compared against orc_commit_rows.
    max_rounds: stop after that many rounds and free the unfinished handle. after_round(k): called after round k's comparison."""
    from spartan_amd import capi
    L = capi.lib
    n = len(a)
    q_idx = g_off + n if q_idx is None else q_idx
    h_idx = g_off + n + 1 if h_idx is None else h_idx
    ipa = vp()
    tab = None
    if dev_extra is None:
        _ok(L.sp_ipa_begin(ctx.h, g.h, sz(g_off), sz(n), sz(q_idx), sz(h_idx), fq1(script["q_scale"]), mont_bulk(a), mont_bulk(b), ctypes.byref(ipa)), "sp_ipa_begin " + tag)
    else:
        rng = random.Random(n + dev_extra)
        blind_a = rng.randrange(1, Q)
        tab = capi.Table.upload(ctx, mont_bulk(a + [rng.randrange(Q) for _ in range(dev_extra)]), n + dev_extra)
        ca = (ctypes.c_uint8 * 32)()
        _ok(L.sp_ipa_begin_dev(ctx.h, g.h, sz(g_off), sz(n), sz(q_idx), sz(h_idx), tab.h, mont_bulk(b), fq1(blind_a), ca, ctypes.byref(ipa)), "sp_ipa_begin_dev " + tag)
        wc = (ctypes.c_uint8 * 32)()
        assert orc.orc_commit_rows(b"".join(P[g_off:g_off + n]), sz(n), P[h_idx], mont_bulk(a), sz(1), sz(n), fq1(blind_a), wc) == 0
        _eq(sec, bytes(ca), bytes(wc), "commit_a " + tag)
        if not prelaunch:
            _ok(L.sp_ipa_set_scale(ipa, fq1(script["q_scale"])), "sp_ipa_set_scale " + tag)
    try:
        k = 0
        for st in script["steps"]:
            if st[0] == "round":
                if k == max_rounds:
                    return
                if prelaunch:      # the kernel goes out before the blinds and the scale of Q are known
                    _ok(L.sp_ipa_round_prelaunch(ipa), "sp_ipa_round_prelaunch " + tag)
                    _ok(L.sp_ipa_set_scale(ipa, fq1(script["q_scale"])), "sp_ipa_set_scale " + tag)
                Lb = (ctypes.c_uint8 * 32)(); Rb = (ctypes.c_uint8 * 32)()
                _ok(L.sp_ipa_round_lr(ipa, fq1(st[1]), fq1(st[2]), Lb, Rb), "sp_ipa_round_lr %s round %d" % (tag, k + 1))
                _eq(sec, bytes(Lb), want["L"][k], "L of round %d %s" % (k + 1, tag))
                _eq(sec, bytes(Rb), want["R"][k], "R of round %d %s" % (k + 1, tag))
                k += 1
                if after_round:
                    after_round(k)
            else:
                _ok(L.sp_ipa_round_fold(ipa, fq1(st[1]), fq1(st[2])), "sp_ipa_round_fold " + tag)
        if max_rounds is not None and k == max_rounds:
            return
        ah = (ctypes.c_uint64 * 4)(); bh = (ctypes.c_uint64 * 4)(); out = (ctypes.c_uint8 * 32)()
        d, r = fq1(script["d"]), fq1(script["r"])
        for call in order:
            if call == "finish_commit":
                _ok(L.sp_ipa_finish_commit(ipa, d, r, ah, bh, out), "sp_ipa_finish_commit " + tag)
                _eq(sec, from_mont_bulk(ah, 1)[0], want["a_hat"], "a_hat of finish_commit " + tag)
                _eq(sec, from_mont_bulk(bh, 1)[0], want["b_hat"], "b_hat of finish_commit " + tag)
                _eq(sec, bytes(out), want["delta"], "delta of finish_commit " + tag)
            elif call == "finish":
                _ok(L.sp_ipa_finish(ipa, ah, bh, out), "sp_ipa_finish " + tag)
                _eq(sec, from_mont_bulk(ah, 1)[0], want["a_hat"], "a_hat of finish " + tag)
                _eq(sec, from_mont_bulk(bh, 1)[0], want["b_hat"], "b_hat of finish " + tag)
                _eq(sec, bytes(out), want["g_hat"], "g_hat " + tag)
            else:
                _ok(L.sp_ipa_commit_ghat(ipa, d, r, out), "sp_ipa_commit_ghat " + tag)
                _eq(sec, bytes(out), want["delta"], "delta of commit_ghat " + tag)
    finally:
        if not _DEVICE_ERROR:
            L.sp_ipa_free(ipa)
            if tab is not None:
                tab.free()


_FOLDED = {}


def folded(key, orc, P, a, b, script, **kw):
    """the folded reference, computed once per key and left unchanged (cases that differ in options only share theirs)"""
    if key not in _FOLDED:
        _FOLDED[key] = I.folded_reference(orc, P, a, b, script, **kw)
    return _FOLDED[key]


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("n0", SIZE_CASES)
def test_every_size_at_which_the_state_machine_changes_path(ctx, orc, gsets, n0, tree):
    g, P = gsets(set_for(n0, tree))
    a, b, sc = size_case(n0, tree)
    drive("sizes", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc), tag="n0=%d %s" % (n0, tree))


# ------------------------------------------------------------------ 2. the row reducer at and above 256 partial sums
@pytest.mark.parametrize("name,ded", REDUCER_CASES)
def test_row_reducer_at_256_partial_sums_and_above(ctx, orc, gsets, name, ded):
    n0 = 4096
    g, P = gsets(name)
    a, b, sc = size_case(n0, name)
    want = folded(("reducer", name), orc, P, a, b, sc)
    with _Options(ctx, ipa__dedicated_uploaded=ded):
        drive("reducer", ctx, orc, g, P, a, b, sc, want, tag="%s dedicated_uploaded=%d" % (name, ded))


# ------------------------------------------------------------------ 3. above 4096
def _msm_launches(ctx):
    return sum(v["launches"] for k, v in ctx.prof_read().items() if k.startswith("msm_"))


@pytest.mark.parametrize("n0,rounds", LARGE_CASES)
def test_openings_above_4096(ctx, orc, gsets, n0, rounds):
    """flat reference (tests/test_ipa_reference.py licenses it; with the rows spread over the cores the three references take 1.3 s, 2.6 s and
    5.2 s on eight cores, 6.9 s and 13.7 s for the first two on one). The call statistics tell the paths apart: a one-launch round is one launch
    of the "ipa" family and none of the msm_* families; a round on k_ipa_prepare is followed by commitment launches (sp_ctx_trips cannot: both
    paths make one trip per round at the sizes that fit the lookup+tree commitment). n0 = 32768 is the case that found msm_launch refusing a
    two-row commitment with per-row generator lists once it has more than 2^19 lookups: every unfused round of such an opening returned
    SP_EINVAL. Those rows now go out one launch each (commit.hip)."""
    g, P = gsets("d32770")
    a, b, sc = large_case(n0)
    want = I.flat_reference(orc, P, a, b, sc, max_rounds=rounds, threads=min(16, os.cpu_count() or 1))
    seen = []

    def after_round(k):
        st = ctx.prof_read()
        seen.append((st["ipa"]["launches"], _msm_launches(ctx)))
        ctx.prof_reset()
    ctx.prof_enable(True); ctx.prof_reset()
    try:
        drive("large", ctx, orc, g, P, a, b, sc, want, max_rounds=rounds, after_round=after_round, tag="n0=%d" % n0)
    finally:
        ctx.prof_enable(False)
    opts = opts_for("d32770")
    ev = [e[1] for e in I.trace(n0, geom_of("d32770").nwin, sc["steps"], opts) if e[0] == "round"][:len(seen)]
    assert len(seen) == (rounds or n0.bit_length() - 1)
    assert seen[0][0] >= 1 and all(s[0] == 1 for s in seen[1:])      # (the first span also holds k_ipa_init)
    assert [s[1] == 0 for s in seen] == [p["fusable"] for p in ev], (seen, [p["fusable"] for p in ev])
    assert all(p["fusable"] for p in ev) if n0 <= 16384 else not any(p["fusable"] for p in ev)


# ------------------------------------------------------------------ 4. values
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("n0", VALUE_N)
def test_edge_values_and_relations(ctx, orc, gsets, n0, tree, fused):
    g, P = gsets(set_for(n0, tree))
    with _Options(ctx, ipa__fused=fused):
        for name in VALUE_CASES:
            a, b, sc = value_case(n0, name)
            want = folded(("value", n0, tree, name), orc, P, a, b, sc)
            if name == "d_r_zero":
                assert want["delta"] == I.NEUTRAL
            drive("values", ctx, orc, g, P, a, b, sc, want, tag="%s n0=%d %s fused=%d" % (name, n0, tree, fused))


# ------------------------------------------------------------------ 5. digits
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("wbits,windows", DIGIT_GEOMS)
def test_signed_digits_of_the_round_kernel_at_every_window_geometry(ctx, orc, gsets, wbits, windows, tree):
    """round 1 has s = [1]: the scalar k_ipa_round recodes is the pool value itself"""
    name = "g%s_%d_%d" % (tree[0], wbits, windows)
    g, P = gsets(name)
    for k, a in enumerate(digit_chunks(geom_of(name))):
        sc = I.make_script(8, random.Random(_seed("digits", name, k)))
        b = [1] * 8
        drive("digits", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc), tag="%s chunk %d" % (name, k))


# ------------------------------------------------------------------ 6. call orders
def test_prelaunch_set_scale_round_through_begin_dev(ctx, orc, gsets):
    n0, name, extra = PRELAUNCH_CASE
    g, P = gsets(name)
    a, b, sc = order_case("prelaunch", n0)
    drive("orders", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc), prelaunch=True, dev_extra=extra, tag="prelaunch")


@pytest.mark.parametrize("n0,at", DOUBLE_FOLD_CASES)
def test_two_folds_with_no_round_between(ctx, orc, gsets, n0, at):
    """not the protocol, but the API allows it (ipa_flush_fold): the model folds twice too"""
    g, P = gsets("d70")
    a, b, sc = order_case("double_fold", n0, double_fold_at=at)
    drive("orders", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc), tag="double fold n0=%d after round %d" % (n0, at))


@pytest.mark.parametrize("order,finish_device", FINISH_CASES)
def test_finishing_calls_in_every_order(ctx, orc, gsets, order, finish_device):
    n0 = 64
    for name in ("d70", "u70"):
        g, P = gsets(name)
        a, b, sc = order_case("finish", n0)
        with _Options(ctx, ipa__finish_device=finish_device):
            drive("orders", ctx, orc, g, P, a, b, sc, folded(("finish", name), orc, P, a, b, sc), order=ORDERS[order], tag="%s %s finish_device=%d" % (order, name, finish_device))


def test_free_over_an_uncollected_prelaunch_leaves_the_context_usable(ctx, orc, gsets):
    from spartan_amd import capi
    L = capi.lib
    g, P = gsets("d70")
    a, b, sc = order_case("free", 64)
    ipa = vp()
    _ok(L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(64), sz(64), sz(65), fq1(sc["q_scale"]), mont_bulk(a), mont_bulk(b), ctypes.byref(ipa)), "sp_ipa_begin")
    _ok(L.sp_ipa_round_prelaunch(ipa), "sp_ipa_round_prelaunch")
    L.sp_ipa_free(ipa)
    rows, cols = 3, 69
    Z, bl = I.edge_vector(rows * cols, random.Random(5)), I.edge_vector(rows, random.Random(6))
    got = g.commit_rows(mont_bulk(Z), rows, cols, mont_bulk(bl), g_off=0, h_idx=69)
    want = (ctypes.c_uint8 * (32 * rows))()
    assert orc.orc_commit_rows(b"".join(P[:cols]), sz(cols), P[69], mont_bulk(Z), sz(rows), sz(cols), mont_bulk(bl), want) == 0
    _eq("orders", got, bytes(want), "commit_rows after sp_ipa_free")
    drive("orders", ctx, orc, g, P, a, b, sc, folded(("free", 64), orc, P, a, b, sc), prelaunch=True, tag="after free")      # and a whole argument


@pytest.mark.parametrize("n0,name", ENCODE_DEVICE_CASES)
def test_every_encode_on_the_device(ctx, orc, gsets, n0, name):
    g, P = gsets(name)
    a, b, sc = order_case("encode_device", n0)
    with _Options(ctx, encode__device=1):
        drive("orders", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc), tag="encode.device n0=%d" % n0)


# ------------------------------------------------------------------ 7. positions
@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("name,g_off,n0,q_idx,h_idx", POSITION_CASES)
def test_generator_positions(ctx, orc, gsets, name, g_off, n0, q_idx, h_idx, tree):
    g, P = gsets(set_for(n0, tree))
    a, b, sc = position_case(name, n0)
    kw = dict(g_off=g_off, q_idx=q_idx, h_idx=h_idx)
    drive("positions", ctx, orc, g, P, a, b, sc, I.folded_reference(orc, P, a, b, sc, **kw), tag="%s %s" % (name, tree), **kw)


# ------------------------------------------------------------------ 8. refusals
def test_refusals_change_nothing(ctx, orc, gsets):
    """every argument check of ipa.hip returns SP_EINVAL before anything is launched; the calls that follow on the same handle still match"""
    from spartan_amd import capi
    L = capi.lib
    g, P = gsets("d70")
    n0 = 4
    a, b, sc = order_case("refusals", n0)
    want = I.folded_reference(orc, P, a, b, sc)
    A, B, qs = mont_bulk(a), mont_bulk(b), fq1(sc["q_scale"])
    big = mont_bulk(a * 32)
    ipa = vp()
    ref = ctypes.byref(ipa)
    for what, rc in [
            ("n0 = 0", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(0), sz(4), sz(5), qs, A, B, ref)),
            ("n0 = 3", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(3), sz(4), sz(5), qs, A, B, ref)),
            ("g_off + n > len", L.sp_ipa_begin(ctx.h, g.h, sz(7), sz(64), sz(4), sz(5), qs, big, big, ref)),
            ("g_off + n > len by one", L.sp_ipa_begin(ctx.h, g.h, sz(67), sz(4), sz(4), sz(5), qs, A, B, ref)),
            ("q_idx = len", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(70), sz(5), qs, A, B, ref)),
            ("h_idx = len", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(4), sz(70), qs, A, B, ref)),
            ("null context", L.sp_ipa_begin(None, g.h, sz(0), sz(4), sz(4), sz(5), qs, A, B, ref)),
            ("null generators", L.sp_ipa_begin(ctx.h, None, sz(0), sz(4), sz(4), sz(5), qs, A, B, ref)),
            ("null scale", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), None, A, B, ref)),
            ("null a", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), qs, None, B, ref)),
            ("null b", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), qs, A, None, ref)),
            ("null out", L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), qs, A, B, None))]:
        _refused(rc, "sp_ipa_begin, " + what)
        assert not ipa.value, what
        COUNTS["refusals"] += 1
    short = capi.Table.upload(ctx, mont_bulk(a[:3]), 3)
    ca = (ctypes.c_uint8 * 32)(*([0xA5] * 32))
    for what, rc in [
            ("a_dev shorter than n", L.sp_ipa_begin_dev(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), short.h, B, qs, ca, ref)),
            ("null a_dev", L.sp_ipa_begin_dev(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), None, B, qs, ca, ref)),
            ("null blind_a", L.sp_ipa_begin_dev(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), short.h, B, None, ca, ref)),
            ("null commit_a", L.sp_ipa_begin_dev(ctx.h, g.h, sz(0), sz(4), sz(4), sz(5), short.h, B, qs, None, ref))]:
        _refused(rc, "sp_ipa_begin_dev, " + what)
        assert not ipa.value and bytes(ca) == bytes([0xA5] * 32), what
        COUNTS["refusals"] += 1
    short.free()
    L.sp_ipa_free(None)      # a null handle: nothing to do
    _refused(L.sp_ipa_round_prelaunch(None), "sp_ipa_round_prelaunch(NULL)")
    _refused(L.sp_ipa_set_scale(None, qs), "sp_ipa_set_scale(NULL)")
    _ok(L.sp_ipa_begin(ctx.h, g.h, sz(0), sz(n0), sz(n0), sz(n0 + 1), qs, A, B, ref), "sp_ipa_begin")
    try:
        Lb = (ctypes.c_uint8 * 32)(); Rb = (ctypes.c_uint8 * 32)(); out = (ctypes.c_uint8 * 32)()
        ah = (ctypes.c_uint64 * 4)(); bh = (ctypes.c_uint64 * 4)()
        rounds = [s for s in sc["steps"] if s[0] == "round"]
        folds = [s for s in sc["steps"] if s[0] == "fold"]
        d, r = fq1(sc["d"]), fq1(sc["r"])

        def finishing_calls_refused(when):
            for what, rc in [("sp_ipa_finish", L.sp_ipa_finish(ipa, ah, bh, out)), ("sp_ipa_finish_commit", L.sp_ipa_finish_commit(ipa, d, r, ah, bh, out)),
                             ("sp_ipa_commit_ghat", L.sp_ipa_commit_ghat(ipa, d, r, out))]:
                _refused(rc, "%s at %s" % (what, when))
                COUNTS["refusals"] += 1
        finishing_calls_refused("n_cur = 4")
        for k in range(2):
            for what, rc in [("null blind_L", L.sp_ipa_round_lr(ipa, None, fq1(1), Lb, Rb)), ("null blind_R", L.sp_ipa_round_lr(ipa, fq1(1), None, Lb, Rb)),
                             ("null L", L.sp_ipa_round_lr(ipa, fq1(1), fq1(1), None, Rb)), ("null R", L.sp_ipa_round_lr(ipa, fq1(1), fq1(1), Lb, None)),
                             ("null handle", L.sp_ipa_round_lr(None, fq1(1), fq1(1), Lb, Rb)), ("null scale", L.sp_ipa_set_scale(ipa, None)),
                             ("fold, null u", L.sp_ipa_round_fold(ipa, None, fq1(1))), ("fold, null u_inv", L.sp_ipa_round_fold(ipa, fq1(1), None)),
                             ("fold, null handle", L.sp_ipa_round_fold(None, fq1(1), fq1(1)))]:
                _refused(rc, "round %d, %s" % (k + 1, what))
                COUNTS["refusals"] += 1
            _ok(L.sp_ipa_round_lr(ipa, fq1(rounds[k][1]), fq1(rounds[k][2]), Lb, Rb), "sp_ipa_round_lr")
            _eq("refusals", bytes(Lb), want["L"][k], "L of round %d after refusals" % (k + 1))
            _eq("refusals", bytes(Rb), want["R"][k], "R of round %d after refusals" % (k + 1))
            _ok(L.sp_ipa_round_fold(ipa, fq1(folds[k][1]), fq1(folds[k][2])), "sp_ipa_round_fold")
            if k == 0:
                finishing_calls_refused("n_cur = 2")
        for what, rc in [("sp_ipa_round_lr", L.sp_ipa_round_lr(ipa, fq1(1), fq1(1), Lb, Rb)), ("sp_ipa_round_fold", L.sp_ipa_round_fold(ipa, fq1(3), fq1(I.INV(3)))),
                         ("sp_ipa_round_prelaunch", L.sp_ipa_round_prelaunch(ipa)),
                         ("sp_ipa_finish, null a_hat", L.sp_ipa_finish(ipa, None, bh, out)), ("sp_ipa_finish_commit, null d", L.sp_ipa_finish_commit(ipa, None, r, ah, bh, out)),
                         ("sp_ipa_finish_commit, null delta", L.sp_ipa_finish_commit(ipa, d, r, ah, bh, None)), ("sp_ipa_commit_ghat, null r", L.sp_ipa_commit_ghat(ipa, d, None, out))]:
            _refused(rc, "%s at n_cur = 1" % what)
            COUNTS["refusals"] += 1
        _ok(L.sp_ipa_finish_commit(ipa, d, r, ah, bh, out), "sp_ipa_finish_commit")
        _eq("refusals", (from_mont_bulk(ah, 1)[0], from_mont_bulk(bh, 1)[0], bytes(out)), (want["a_hat"], want["b_hat"], want["delta"]), "finish_commit after refusals")
        _ok(L.sp_ipa_finish(ipa, ah, bh, out), "sp_ipa_finish")
        _eq("refusals", (from_mont_bulk(ah, 1)[0], from_mont_bulk(bh, 1)[0], bytes(out)), (want["a_hat"], want["b_hat"], want["g_hat"]), "finish after refusals")
    finally:
        if not _DEVICE_ERROR:
            L.sp_ipa_free(ipa)
