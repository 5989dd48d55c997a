"""The F_q streaming kernels (spartan_amd/csrc/fq_ops.hip: the eq tables, the sum-check evaluate / bind kernels of the ZK sum-checks and
their tiny form, bind-top, k_reduce_partials and the host-side sums, vector x matrix, dot, evaluate, the gather / split / pack helpers) on
FIELD EDGE VALUES and at EVERY BOUNDARY OF THEIR HOST-SIDE DISPATCH. tests/test_gpu_large.py holds the throughput shapes on uniform random
scalars; here the tables are made of the Fq edge pool (layout a: neighbouring lanes differ; layout c: a whole wavefront of one value),
challenges cycle through 0, one, q - 1 and a random residue (whole terms vanish; the tiny kernels and k_eq_expand_small choose their
operands by per-limb selects), one table per set has equal halves, and the case lists below sit on the thresholds of the dispatch:

  partial sums added by the host (up to 960) or by k_reduce_partials (sum-checks from 2^18 / 2^19, dot from 245761); one or two grid-stride
  passes (half, quarter = 2^19; dot at 262145); the tiny form from quarter 8192 down to a partly live block, the streaming form above it and
  for kind 1 at every length; the challenge vector of the eq kernel in the kernel arguments or staged, with 0..5 high bits, and the outer
  product of two short tables; the 8-slot ring of sp_eq_expand wrapped without a wait; sp_vecmat off the powers of two, at 8 and 9 row
  chunks and on both sides of 2^22 elements; the 1024 entries of the result area; every TOPB form of k_evaluate.

tests/test_fq_reference.py asserts on the CPU (through fq_reference.plan) that the lists reach each of these and that no compared sum is
blind to an index at a block, pass or table boundary. Expected values: the Python-integer models of tests/fq_reference.py, which that
module checks against the oracle; the one case whose model would take too long says so. Every comparison is an exact integer comparison of
every output word and every downloaded table entry, and every value the device returns must be below q. After a SpartanHipError or an
unexpected status nothing further is started. The list of such errors is the one of tests/test_gpu_spark_edges.py, whose helpers this
module uses: a device error in either module also stops the other ("not started: an earlier call failed on the device"), since
what follows a failed call on a shared GPU proves nothing and may do harm.

Not reached here: sp_eq_expand at ell 27..32 (tables of 4 GiB and more), the only calls whose upper half has 14..16 variables; that half
fills r[13..15] of k_eq_expand_small and is read from the staged slot whatever sumcheck.inline_args says. The bound of 32 is tested as
a refusal at 33 only."""
import ctypes, functools, random
import pytest
from tests import field_vectors as V
from tests import fq_reference as F
from tests.helpers import Q, vp, sz, gens_bytes
from tests import test_gpu_spark_edges as E
from tests.test_gpu_spark_edges import _DEVICE_ERROR, _flags_device_errors, _ok, _refused, _arr, _ints, _handles
from tests.test_gpu_spark_edges import _nothing_after_a_device_error      # the autouse guard: a fixture of this module too

pytestmark = pytest.mark.gpu

ZERO, ONE, MINUS = 0, F.ONE, Q - 1

# ------------------------------------------------------------------ the case lists (imported by tests/test_fq_reference.py: no GPU needed)
# eq: every ell, on a context with sumcheck.inline_args at 1 and on one with 0; the challenge vectors of every case
EQ_ELLS = list(range(1, 14)) + [14, 15, 17]
EQ_VECTORS = ["zero", "one", "minus", "cycle", "random"]      # all 0 and all one make one-hot tables
EQ_RING_ELL, EQ_RING_CALLS = 14, 10
EQ_REFUSED = [0, 33, 41]
# chains: (kind, len0, layout, base, cstart): table j of the set is edge_table(layout, len0, base + j), table 1 with equal halves; the
# challenge of round j is cycle[(cstart + j) % 4] of (0, one, q - 1, random). No challenge here removes a term from a compared sum: a bind
# at 0 or one selects a half of every table, and the sums are taken over what is left.
CHAIN_CASES = [(0, 1 << 16, "a", 0, 0), (0, 1 << 16, "c", 5, 3), (2, 1 << 16, "a", 8, 3), (2, 1 << 16, "c", 13, 0),
               (1, 1 << 12, "a", 16, 0), (1, 1 << 12, "c", 20, 2)]
# single rounds: (call, kind, length, layout, base, index of r in the cycle or None, where the expected values come from)
ROUND_CASES = (
    [("sc_eval", k, n, "a", 24 + 4 * k, None, "model") for k in (0, 1, 2) for n in (1 << 17, 1 << 18)] +
    [("sc_bind_eval", k, 1 << 18, "a", 37 + 4 * k, 2, "model") for k in (0, 1, 2)] +
    [("sc_bind_eval", k, 1 << 19, "c" if k == 0 else "a", 48 + 4 * k, 3, "model") for k in (0, 1, 2)] +
    [("sc_eval", 0, 1 << 20, "a", 60, None, "model"),            # grid-stride: a second pass from half = 2^19
     ("sc_bind_eval", 0, 1 << 21, "a", 64, 3, "oracle")])        # ... from quarter = 2^19
# sp_sumcheck_bind_eval_commit: (kind, length, rows, layout, base, index of r)
# (the third: the tables and challenge of the round case at 2^19, kind 0: 512 blocks, their sums added by k_reduce_partials)
COMMIT_CASES = [(2, 4 * 8192, 8, "a", 68, 3), (1, 4, 1, "a", 72, 2), (0, 1 << 19, 1, "c", 48, 3)]
# records and round trips per call: (kind, length) at the smallest shape of each plan - tiny with host sums, streaming with host sums,
# streaming with device sums by the _start rule alone (3 blocks), streaming with device sums (512 blocks)
RECORD_SHAPES = [(2, 4 * 8192), (1, 4), (1, 1 << 12), (0, 1 << 19)]
RECORD_CALLS = ["eval", "bind_eval", "start", "commit"]
DOT_N = [1, 255, 256, 257, 245760, 245761, 262144, 262145]
DOT_OFF = (3, 5)            # a_off, b_off
DOT_BASE = 76
# evaluate: "cycle": r_k = cycle[k % 4]: a coordinate at 0 removes the half of the table whose index bit is set, one at one the other half
# (the boundary-term condition of tests/test_fq_reference.py is exempt for those halves only); "dense": no coordinate is 0 or one
EVAL_ELLS = [1, 2, 3, 4, 5, 12, 13]
EVAL_VECTORS = ["cycle", "dense"]
EVAL_BASE = 82
VECMAT_CASES = [(1, 1), (1, 65), (3, 63), (4, 64), (16, 64), (17, 33), (128, 32), (129, 31), (64, 65536), (65, 64531)]
VECMAT_DEV_CASES = [(17, 33), (129, 31)]      # also through sp_vecmat_dev and sp_vecmat_tab
BIND_TOP_CASES = [(nt, n) for nt in (1, 4, 5, 9) for n in (2, 1024)]
HEADS_CASES = [1, 256, 257, 1024]
SPLIT_LENS = [1, 257, 771, 1024]              # 771 = 3 * 257: the one length here that W = 3 divides
SPLIT_W = [1, 3, 4, "len"]

COUNTS = {k: 0 for k in ("eq", "chain", "round", "commit", "dot", "evaluate", "vecmat", "bind", "heads", "copy")}      # exact comparisons per section


def challenge_vector(kind, ell, seed=0):
    cyc = F.edge_challenges(1000 + ell + seed)
    if kind == "dense":
        rng = random.Random(2000 + ell + seed)
        return [MINUS if k % 3 == 0 else rng.randrange(2, Q) for k in range(ell)]
    return {"zero": [ZERO] * ell, "one": [ONE] * ell, "minus": [MINUS] * ell, "cycle": [cyc[k % 4] for k in range(ell)],
            "random": [random.Random(3000 + ell + seed + k).randrange(Q) for k in range(ell)]}[kind]


def case_tables(kind, layout, n, base):
    """the tables of a sum-check case; table 1 has equal halves (x1 - x0 = 0 in every pair of the first round)"""
    T = [F.edge_table(layout, n, base + j) for j in range(F.NTABS[kind])]
    if n >= 4:
        T[1] = T[1][:n // 2] * 2
    return T


def case_tables_raw(kind, layout, n, base):
    raw = [F.edge_table_bytes(layout, n, base + j) for j in range(F.NTABS[kind])]
    if n >= 4:
        raw[1] = raw[1][:16 * n] * 2
    return raw


def case_r(length, kind, ridx):
    return F.edge_challenges(length + kind)[ridx]


@functools.lru_cache(maxsize=None)
def chain_model(kind, len0, layout, base, cstart):
    """[(r, tables, evaluations)]: entry 0 the tables as uploaded (r None), entry j + 1 after the bind at challenge j; the evaluations are
    None once a single entry is left. Computed once and shared; nobody changes it."""
    T = case_tables(kind, layout, len0, base)
    cyc = F.edge_challenges(len0 + kind)
    rounds, j = [(None, T, F.sc_evals(kind, T))], cstart
    while len(T[0]) >= 2:
        r = cyc[j % 4]; j += 1
        T = [F.bind(t, r) for t in T]
        rounds.append((r, T, F.sc_evals(kind, T) if len(T[0]) >= 2 else None))
    return rounds


# ------------------------------------------------------------------ fixtures and comparison helpers
@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    if _DEVICE_ERROR:     # module fixtures are set up before the function-scoped guard above
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    c = capi.Ctx(0)
    yield c
    c.close()
    chain_model.cache_clear(); _chi.cache_clear(); _edge.cache_clear()
    print("\nexact comparisons per section: %s" % ", ".join("%s %d" % kv for kv in sorted(COUNTS.items())))


@pytest.fixture(scope="module")
def ctx_staged(ctx):
    """a context of its own with sumcheck.inline_args = 0: the eq kernel reads its challenge vector from the host-mapped page"""
    from spartan_amd import capi
    c = capi.Ctx(0)
    c.set_option("testing.unlock", 1)
    c.set_option("sumcheck.inline_args", 0)
    yield c
    c.close()


def _same(sec, got, want, what):
    """exact comparison of every value, each below q (the SPARK module's, counted here)"""
    E._same(sec, got, want, what, COUNTS)


def _same_raw(sec, t, want_raw, what, off=0):
    """the table's contents against packed expected values (below q by construction: equal bytes are reduced values)"""
    n = len(want_raw) // 32
    raw = bytes(t.download(n, off))
    if raw != want_raw:
        _same(sec, _ints(raw), _ints(want_raw), what)
    COUNTS[sec] += n


def _same_table(sec, t, want, what, off=0):
    _same_raw(sec, t, V.pack(want), what, off)


@functools.lru_cache(maxsize=None)
def _edge(layout, n, k):
    return F.edge_table(layout, n, k), F.edge_table_bytes(layout, n, k)


@functools.lru_cache(maxsize=None)
def _chi(kind, ell, seed=0):
    r = challenge_vector(kind, ell, seed)
    return r, V.pack(F.chi(r))


def _up(ctx, vals=None, raw=None):
    from spartan_amd import capi
    raw = V.pack(vals) if raw is None else raw
    return capi.Table.upload(ctx, raw, len(raw) // 32)


def _free(tabs):
    for t in tabs:
        t.free()


# ------------------------------------------------------------------ eq tables
@pytest.mark.parametrize("inline", [1, 0])
@pytest.mark.parametrize("ell", EQ_ELLS)
@_flags_device_errors
def test_eq_tables_at_every_ell_and_challenge_transport(ctx, ctx_staged, ell, inline):
    """sp_eq_expand against chi(r) for r all 0, all one (one-hot tables), all q - 1, the four-cycle and random: ell 1, 2 and 7 have nb = 0 or
    na != nb, 8 against 9 is no high bit against one, 13 is five; 14, 15 and 17 are outer products of two short tables (7 x 7, 8 x 7, 9 x 8)"""
    from spartan_amd import capi
    c = ctx if inline else ctx_staged
    for kind in EQ_VECTORS:
        r, want = _chi(kind, ell)
        t = capi.Table.eq(c, _arr(r), ell)
        assert len(t) == 1 << ell
        _same_raw("eq", t, want, "sp_eq_expand ell=%d r %s inline_args=%d" % (ell, kind, inline))
        t.free()


@pytest.mark.parametrize("inline", [0, 1])
@_flags_device_errors
def test_eq_ring_wrapped_without_a_wait(ctx, ctx_staged, inline):
    """ten calls at ell = 14 with ten vectors before anything is downloaded: the ninth takes the first call's slot of the 8-slot ring.
    inline = 0 is the case that can see a ring defect: on that context both launches of every call read their challenges from the call's
    slot (the lower half at an offset of hi_ell scalars), so a wrong slot index, stride, offset or reuse rule gives a wrong table. With
    inline = 1 both halves (7 variables each) travel in the kernel arguments and nobody reads the slots: that run only shows that taking
    and re-taking slots, with the wait the ninth call makes, does not disturb the tables."""
    from spartan_amd import capi
    c = ctx if inline else ctx_staged
    vecs = [challenge_vector("random", EQ_RING_ELL, seed=100 + k) for k in range(EQ_RING_CALLS)]
    vecs[3] = challenge_vector("cycle", EQ_RING_ELL); vecs[8] = challenge_vector("minus", EQ_RING_ELL)
    tabs = [capi.Table.eq(c, _arr(r), EQ_RING_ELL) for r in vecs]
    for k, (t, r) in enumerate(zip(tabs, vecs)):
        _same_table("eq", t, F.chi(r), "table %d of %d back-to-back sp_eq_expand calls, inline_args=%d" % (k, EQ_RING_CALLS, inline))
    _free(tabs)


@_flags_device_errors
def test_eq_refuses_what_its_kernel_cannot_hold(ctx):
    """ell = 0, and ell = 33 and 41: a long table's upper half has ell - ell/2 variables and k_eq_expand_small holds 16. Refused before
    anything is allocated (2^33 entries are 256 GiB): the handle stays null."""
    from spartan_amd import capi
    r = _arr(challenge_vector("random", 41))
    for ell in EQ_REFUSED:
        h = vp()
        _refused(capi.lib.sp_eq_expand(ctx.h, r, sz(ell), ctypes.byref(h)), "sp_eq_expand ell=%d" % ell)
        assert not h.value, ell
    t = capi.Table.eq(ctx, r, 3)      # the context goes on working
    _same_table("eq", t, F.chi(challenge_vector("random", 41)[:3]), "sp_eq_expand after the refusals")
    t.free()


# ------------------------------------------------------------------ sum-check chains
@pytest.mark.parametrize("mode", ["fused", "start"])
@pytest.mark.parametrize("kind,len0,layout,base,cstart", CHAIN_CASES)
@_flags_device_errors
def test_sumcheck_chain_down_to_the_heads(ctx, kind, len0, layout, base, cstart, mode):
    """sp_sumcheck_eval at every length, then the bind and the next evaluation through sp_sumcheck_bind_eval ("fused") or through
    sp_sumcheck_bind_eval_start / _collect ("start"), down to length 2: there the fused call must refuse and leave the tables alone, and
    sp_table_bind_top_heads does the last round. Kinds 0 and 2 from 2^16: one streaming round, then the tiny form from 256 blocks down to
    one partly live block; kind 1 from 2^12: streaming at every length. After every round: the evaluations and every table in full."""
    from spartan_amd import capi
    L = capi.lib
    rounds = chain_model(kind, len0, layout, base, cstart)
    nt, nv = F.NTABS[kind], len(F.POINTS[kind])
    tabs = [_up(ctx, raw=raw) for raw in case_tables_raw(kind, layout, len0, base)]
    h = _handles(tabs)
    out = (ctypes.c_uint64 * 12)()
    for j in range(len(rounds) - 1):
        _, T, ev = rounds[j]
        length = len(T[0])
        r, Tn, evn = rounds[j + 1]
        what = "kind %d len0=%d layout %s %s at length %d" % (kind, len0, layout, mode, length)
        _ok(L.sp_sumcheck_eval(ctx.h, ctypes.c_int(kind), h, sz(nt), out), "sp_sumcheck_eval " + what)
        _same("chain", _ints(out, nv), ev, "sp_sumcheck_eval " + what)
        if length >= 4:
            if mode == "fused":
                _ok(L.sp_sumcheck_bind_eval(ctx.h, ctypes.c_int(kind), h, sz(nt), _arr([r]), out), "sp_sumcheck_bind_eval " + what)
            else:
                _ok(L.sp_sumcheck_bind_eval_start(ctx.h, ctypes.c_int(kind), h, sz(nt), _arr([r])), "sp_sumcheck_bind_eval_start " + what)
                _ok(L.sp_sumcheck_bind_eval_collect(ctx.h, out), "sp_sumcheck_bind_eval_collect " + what)
            _same("chain", _ints(out, nv), evn, "bind at r=%#x and evaluate, %s" % (r, what))
        else:
            _refused(L.sp_sumcheck_bind_eval(ctx.h, ctypes.c_int(kind), h, sz(nt), _arr([r]), out), "sp_sumcheck_bind_eval at length 2")
            _refused(L.sp_sumcheck_bind_eval_start(ctx.h, ctypes.c_int(kind), h, sz(nt), _arr([r])), "sp_sumcheck_bind_eval_start at length 2")
            for k, t in enumerate(tabs):
                assert len(t) == 2
                _same_table("chain", t, T[k], "table %d after the refused calls, %s" % (k, what))
            heads = (ctypes.c_uint64 * (4 * nt))()
            _ok(L.sp_table_bind_top_heads(ctx.h, h, sz(nt), _arr([r]), heads), "sp_table_bind_top_heads " + what)
            _same("chain", _ints(heads, nt), [t[0] for t in Tn], "heads of the last round r=%#x, %s" % (r, what))
        for k, t in enumerate(tabs):
            assert len(t) == length // 2, (k, what)
            _same_table("chain", t, Tn[k], "table %d bound at r=%#x from %s" % (k, r, what))
    _free(tabs)


# ------------------------------------------------------------------ single rounds: the host-sum limit and the second grid-stride pass
def _oracle_round(orc, kind, raws, n, r):
    """orc_bound_top on every table and orc_sumcheck_eval on the results, on the same residues"""
    bound = []
    for raw in raws:
        z = (ctypes.c_uint64 * (4 * n)).from_buffer_copy(raw)
        orc.orc_bound_top(z, sz(n), _arr([r]))
        bound.append(z)
    w = (ctypes.c_uint64 * 12)()
    a = bound + [None] * (4 - len(bound))
    orc.orc_sumcheck_eval(ctypes.c_int(kind), a[0], a[1], a[2], a[3], sz(n // 2), w)
    return [bytes(z)[:16 * n] for z in bound], _ints(w, len(F.POINTS[kind]))


@pytest.mark.parametrize("call,kind,length,layout,base,ridx,source", ROUND_CASES)
@_flags_device_errors
def test_single_rounds_above_the_host_sum_limit(ctx, orc, call, kind, length, layout, base, ridx, source):
    """sp_sumcheck_eval at 2^17 (256 blocks: their 768 sums added by the host) and 2^18 (512 blocks: k_reduce_partials), sp_sumcheck_bind_eval
    at 2^18 and 2^19 likewise, every kind; and for kind 0 the lengths 2^20 / 2^21 from which the 1024 blocks make a second grid-stride pass.
    The expected values of the 2^21 round come from the ORACLE (orc_bound_top and orc_sumcheck_eval on the same residues), not from the
    Python model, which takes about 5 s for it; tests/test_fq_reference.py ties the two together at small sizes."""
    from spartan_amd import capi
    L = capi.lib
    nt, nv = F.NTABS[kind], len(F.POINTS[kind])
    raws = case_tables_raw(kind, layout, length, base)
    tabs = [_up(ctx, raw=raw) for raw in raws]
    h = _handles(tabs)
    out = (ctypes.c_uint64 * 12)()
    what = "%s kind %d length %d layout %s" % (call, kind, length, layout)
    if call == "sc_eval":
        _ok(L.sp_sumcheck_eval(ctx.h, ctypes.c_int(kind), h, sz(nt), out), what)
        _same("round", _ints(out, nv), F.sc_evals(kind, case_tables(kind, layout, length, base)), what)
        assert all(len(t) == length for t in tabs)
    else:
        r = case_r(length, kind, ridx)
        if source == "oracle":
            want_tabs, want = _oracle_round(orc, kind, raws, length, r)
        else:
            T = [F.bind(t, r) for t in case_tables(kind, layout, length, base)]
            want_tabs, want = [V.pack(t) for t in T], F.sc_evals(kind, T)
        _ok(L.sp_sumcheck_bind_eval(ctx.h, ctypes.c_int(kind), h, sz(nt), _arr([r]), out), what)
        _same("round", _ints(out, nv), want, "%s r=%#x (expected values from the %s)" % (what, r, source))
        for k, t in enumerate(tabs):
            assert len(t) == length // 2, (k, what)
            _same_raw("round", t, want_tabs[k], "table %d after %s r=%#x" % (k, what, r))
    _free(tabs)


# ------------------------------------------------------------------ the ZK round body
@pytest.mark.parametrize("kind,length,rows,layout,base,ridx", COMMIT_CASES)
@_flags_device_errors
def test_round_body_with_commitments(ctx, orc, kind, length, rows, layout, base, ridx):
    """sp_sumcheck_bind_eval_commit: the evaluations and every table as for the fused call, and the `rows` commitments of the side stream
    against the oracle's orc_pt_msm over the same generators and residues (kind 2 at quarter 8192: the largest tiny round, 8 rows: the row
    sums fill the last KiB of the result area; kind 1 at quarter 1: one row; kind 0 at quarter 2^17: 512 blocks, whose 49152 bytes of sums
    are past what the host adds, so the call launches k_reduce_partials without a signal of its own and waits for both streams at once)"""
    from spartan_amd import capi
    pts = gens_bytes(orc, 39)      # 40 points: G[0..39), h = P[39]
    g = capi.Gens(ctx, compressed=pts)
    nt, nv = F.NTABS[kind], len(F.POINTS[kind])
    idx = [3, 4, 5, 6, 39, 0, 39, 17, 38, 1, 2][:11 if rows > 1 else 4]
    cols = len(idx)
    Sc = F.edge_table("a", rows * cols, base + 5)
    Sc[0] = 0
    r = case_r(length, kind, ridx)
    T = [F.bind(t, r) for t in case_tables(kind, layout, length, base)]
    tabs = [_up(ctx, raw=raw) for raw in case_tables_raw(kind, layout, length, base)]
    ev = (ctypes.c_uint64 * 12)(); out_pts = (ctypes.c_uint8 * (32 * rows))()
    what = "sp_sumcheck_bind_eval_commit kind %d length %d rows %d" % (kind, length, rows)
    _ok(capi.lib.sp_sumcheck_bind_eval_commit(ctx.h, ctypes.c_int(kind), _handles(tabs), sz(nt), _arr([r]), ev, g.h, (ctypes.c_uint32 * cols)(*idx), sz(cols),
                                              _arr(Sc), sz(rows), out_pts), what)
    _same("commit", _ints(ev, nv), F.sc_evals(kind, T), what)
    for k, t in enumerate(tabs):
        assert len(t) == length // 2
        _same_table("commit", t, T[k], "table %d after %s" % (k, what))
    sel = b"".join(pts[32 * i:32 * i + 32] for i in idx)
    for k in range(rows):
        o = (ctypes.c_uint8 * 32)()
        assert orc.orc_pt_msm(_arr(Sc[k * cols:(k + 1) * cols]), sel, sz(cols), o) == 1
        assert bytes(out_pts)[32 * k:32 * k + 32] == bytes(o), ("commitment of row %d, %s" % (k, what))
        COUNTS["commit"] += 1
    _free(tabs); g.free()


# ------------------------------------------------------------------ what a single round call leaves behind
# (call, kind, length) -> (round trips by sp_ctx_trips: of "start" those of _start and of _collect, {profile family: (records, alg_bytes)}
# of every family the call left a record in).
# MEASURED, not derived from the code under test: this test printed the table on the library as it stood before the single round calls
# were given one plan and one launch path, and it was written down here as literals. The calls must go on leaving exactly this behind.
CALL_RECORDS = {
    ('eval', 2, 32768): ((1,), {'sumcheck_eval': (1, 4194304.0)}),
    ('bind_eval', 2, 32768): ((1,), {'sumcheck_bind_eval': (1, 6291456.0)}),
    ('start', 2, 32768): ((0, 1), {'sumcheck_bind_eval': (1, 6291456.0)}),
    ('commit', 2, 32768): ((1,), {'msm_windows_fixed': (1, 256.0), 'sumcheck_bind_eval': (1, 6291456.0)}),
    ('eval', 1, 4): ((1,), {'sumcheck_eval': (1, 384.0)}),
    ('bind_eval', 1, 4): ((1,), {'sumcheck_bind_eval': (1, 576.0)}),
    ('start', 1, 4): ((0, 1), {'sumcheck_bind_eval': (1, 576.0), 'fq_reduce': (1, 96.0)}),
    ('commit', 1, 4): ((1,), {'msm_windows_fixed': (1, 256.0), 'sumcheck_bind_eval': (1, 576.0)}),
    ('eval', 1, 4096): ((1,), {'sumcheck_eval': (1, 393216.0)}),
    ('bind_eval', 1, 4096): ((1,), {'sumcheck_bind_eval': (1, 589824.0)}),
    ('start', 1, 4096): ((0, 1), {'sumcheck_bind_eval': (1, 589824.0), 'fq_reduce': (1, 384.0)}),
    ('commit', 1, 4096): ((1,), {'msm_windows_fixed': (1, 256.0), 'sumcheck_bind_eval': (1, 589824.0)}),
    ('eval', 0, 524288): ((1,), {'sumcheck_eval': (1, 33554432.0), 'fq_reduce': (1, 98304.0)}),
    ('bind_eval', 0, 524288): ((1,), {'sumcheck_bind_eval': (1, 50331648.0), 'fq_reduce': (1, 49152.0)}),
    ('start', 0, 524288): ((0, 1), {'sumcheck_bind_eval': (1, 50331648.0), 'fq_reduce': (1, 49152.0)}),
    ('commit', 0, 524288): ((1,), {'msm_windows_fixed': (1, 256.0), 'sumcheck_bind_eval': (1, 50331648.0), 'fq_reduce': (1, 49152.0)}),
}


@_flags_device_errors
def test_records_and_round_trips_of_every_single_round_call(ctx, orc):
    """sp_sumcheck_eval, sp_sumcheck_bind_eval, sp_sumcheck_bind_eval_start + _collect and sp_sumcheck_bind_eval_commit (one row of four
    columns) at each of RECORD_SHAPES: the round trips each call makes and the profile records it leaves (how many per family, and their
    algorithmic bytes) are those of CALL_RECORDS - one trip per call (at _collect for the split form), one sumcheck record per round, one
    fq_reduce record exactly where the sums are added on the device, the commitment's records next to them."""
    from spartan_amd import capi
    L = capi.lib
    g = capi.Gens(ctx, compressed=gens_bytes(orc, 39))
    idx, Sc = (ctypes.c_uint32 * 4)(3, 4, 5, 6), _arr(F.edge_table("a", 4, 157))
    out, out_pts = (ctypes.c_uint64 * 12)(), (ctypes.c_uint8 * 32)()
    got = {}
    ctx.prof_enable(True)
    try:
        for kind, length in RECORD_SHAPES:
            nt, r = F.NTABS[kind], _arr([case_r(length, kind, 3)])
            for call in RECORD_CALLS:
                tabs = [_up(ctx, raw=raw) for raw in case_tables_raw(kind, "a", length, 150)]
                h, k, what = _handles(tabs), ctypes.c_int(kind), "%s kind %d length %d" % (call, kind, length)
                ctx.prof_reset()
                trips = [L.sp_ctx_trips(ctx.h)]
                if call == "eval":
                    _ok(L.sp_sumcheck_eval(ctx.h, k, h, sz(nt), out), what)
                elif call == "bind_eval":
                    _ok(L.sp_sumcheck_bind_eval(ctx.h, k, h, sz(nt), r, out), what)
                elif call == "start":
                    _ok(L.sp_sumcheck_bind_eval_start(ctx.h, k, h, sz(nt), r), what)
                    trips.append(L.sp_ctx_trips(ctx.h))
                    _ok(L.sp_sumcheck_bind_eval_collect(ctx.h, out), what + " (collect)")
                else:
                    _ok(L.sp_sumcheck_bind_eval_commit(ctx.h, k, h, sz(nt), r, out, g.h, idx, sz(4), Sc, sz(1), out_pts), what)
                trips.append(L.sp_ctx_trips(ctx.h))
                rec = {n: (v["launches"], v["alg_bytes"]) for n, v in ctx.prof_read().items() if v["launches"] or v["alg_bytes"]}
                got[(call, kind, length)] = (tuple(b - a for a, b in zip(trips, trips[1:])), rec)
                _free(tabs)
    finally:
        ctx.prof_enable(False)
    g.free()
    for key in got:
        print("    %r: %r," % (key, got[key]))
    assert got == CALL_RECORDS


# ------------------------------------------------------------------ dot and evaluate
@pytest.mark.parametrize("n", DOT_N)
@_flags_device_errors
def test_dot_at_block_reduce_and_stride_boundaries(ctx, n):
    """sp_dot with both offsets non-zero: one block (1..256), two (257), 960 blocks host-summed (245760), 961 through k_reduce_partials,
    1024 blocks in one pass (262144) and with a second pass of one index (262145); refused past either table's capacity and at n = 0"""
    from spartan_amd import capi
    ao, bo = DOT_OFF
    (A, ra), (B, rb) = _edge("a", n + ao, DOT_BASE), _edge("c", n + bo, DOT_BASE + 1)
    ta, tb = _up(ctx, raw=ra), _up(ctx, raw=rb)
    o = (ctypes.c_uint64 * 4)()
    _ok(capi.lib.sp_dot(ctx.h, ta.h, sz(ao), tb.h, sz(bo), sz(n), o), "sp_dot n=%d" % n)
    _same("dot", _ints(o), [F.dot(A[ao:], B[bo:])], "sp_dot n=%d a_off=%d b_off=%d" % (n, ao, bo))
    _refused(capi.lib.sp_dot(ctx.h, ta.h, sz(ao + 1), tb.h, sz(bo), sz(n), o), "sp_dot with a_off + n = cap + 1")
    _refused(capi.lib.sp_dot(ctx.h, ta.h, sz(ao), tb.h, sz(bo + 1), sz(n), o), "sp_dot with b_off + n = cap + 1")
    _refused(capi.lib.sp_dot(ctx.h, ta.h, sz(ao), tb.h, sz(bo), sz(0), o), "sp_dot with n = 0")
    _free([ta, tb])


@pytest.mark.parametrize("vec", EVAL_VECTORS)
@pytest.mark.parametrize("ell", EVAL_ELLS)
@_flags_device_errors
def test_evaluate_at_every_top_bit_form(ctx, ell, vec):
    """sp_evaluate: ell 1, 2, 3 are k_evaluate<1>, <2>, <3> with one thread; 4 and 5 are <4> with one and two threads; 12 is one full block,
    13 two blocks"""
    from spartan_amd import capi
    Z, raw = _edge("a" if ell % 2 else "c", 1 << ell, EVAL_BASE + ell)
    r = challenge_vector(vec, ell)
    t = _up(ctx, raw=raw)
    o = (ctypes.c_uint64 * 4)()
    _ok(capi.lib.sp_evaluate(ctx.h, t.h, _arr(r), sz(ell), o), "sp_evaluate ell=%d r %s" % (ell, vec))
    _same("evaluate", _ints(o), [F.evaluate(Z, r)], "sp_evaluate ell=%d r %s" % (ell, vec))
    t.free()


# ------------------------------------------------------------------ vector x matrix
@pytest.mark.parametrize("Lsz,R", VECMAT_CASES)
@_flags_device_errors
def test_vecmat_off_the_powers_of_two(ctx, Lsz, R):
    """sp_vecmat with Lsz below, at and off a multiple of its row chunk (16; 32 above 2^22 elements: 64 x 65536 is the last shape of the
    first kind, 65 x 64531 among the first of the second, with a last chunk of one row), R below, at and off 64 and 32, 8 and 9 chunks
    (128 and 129 rows: k_colsum's eight lanes take one chunk each, then lane 0 a second); L holds 0, one and q - 1 where it is long enough.
    Two shapes also through sp_vecmat_dev and sp_vecmat_tab, which leave the result on the device."""
    from spartan_amd import capi
    Z, raw = _edge("a", Lsz * R, 90)
    Lv = list(F.edge_table("a", Lsz, 91))
    for k, x in enumerate((MINUS, ONE, ZERO)):
        if Lsz > k + 1:
            Lv[k + 1] = x
    want = F.vecmat(Lv, Z, R)
    tz = _up(ctx, raw=raw)
    o = (ctypes.c_uint64 * (4 * R))()
    _ok(capi.lib.sp_vecmat(ctx.h, _arr(Lv), sz(Lsz), tz.h, o), "sp_vecmat %d x %d" % (Lsz, R))
    _same("vecmat", _ints(o, R), want, "sp_vecmat %d x %d" % (Lsz, R))
    if (Lsz, R) in VECMAT_DEV_CASES:
        h = vp()
        _ok(capi.lib.sp_vecmat_dev(ctx.h, _arr(Lv), sz(Lsz), tz.h, ctypes.byref(h)), "sp_vecmat_dev %d x %d" % (Lsz, R))
        t = capi.Table(ctx, h)
        assert len(t) == R
        _same_table("vecmat", t, want, "sp_vecmat_dev %d x %d" % (Lsz, R))
        t.free()
        tl, h = _up(ctx, Lv), vp()
        _ok(capi.lib.sp_vecmat_tab(ctx.h, tl.h, tz.h, ctypes.byref(h)), "sp_vecmat_tab %d x %d" % (Lsz, R))
        tl.free()      # L may be freed right after the call
        t = capi.Table(ctx, h)
        assert len(t) == R
        _same_table("vecmat", t, want, "sp_vecmat_tab %d x %d" % (Lsz, R))
        t.free()
    tz.free()


# ------------------------------------------------------------------ bind-top and the heads
@pytest.mark.parametrize("ntabs,n", BIND_TOP_CASES)
@_flags_device_errors
def test_bind_top_in_groups_of_four(ctx, ntabs, n):
    """sp_table_bind_top on 1, 4, 5 and 9 tables (one, one full, two and three launches) at each challenge of the cycle"""
    from spartan_amd import capi
    for j, r in enumerate(F.edge_challenges(ntabs + n)):
        T = [_edge("a" if k % 2 else "c", n, 100 + k + 9 * j) for k in range(ntabs)]
        tabs = [_up(ctx, raw=raw) for _, raw in T]
        _ok(capi.lib.sp_table_bind_top(ctx.h, _handles(tabs), sz(ntabs), _arr([r])), "sp_table_bind_top ntabs=%d n=%d" % (ntabs, n))
        for k, t in enumerate(tabs):
            assert len(t) == n // 2
            _same_table("bind", t, F.bind(T[k][0], r), "table %d of %d bound at r=%#x, n=%d" % (k, ntabs, r, n))
        _free(tabs)


def _bind_top_refusals(ctx, lists_of):
    """each list must be refused with every table's length and contents as they were; then the five tables are bound as usual"""
    from spartan_amd import capi
    n = 1024
    T = [_edge("a", n, 120 + k) for k in range(5)]
    others = {"odd": _edge("a", n // 2, 125), "six": _edge("a", 6, 126)}
    rv = F.edge_challenges(5)[3]
    tabs = [_up(ctx, raw=raw) for _, raw in T]
    extra = {k: _up(ctx, raw=v[1]) for k, v in others.items()}
    for what, picks in lists_of:
        lst = [tabs[p] if isinstance(p, int) else extra[p] for p in picks]
        vals = [T[p][0] if isinstance(p, int) else others[p][0] for p in picks]
        _refused(capi.lib.sp_table_bind_top(ctx.h, _handles(lst), sz(len(lst)), _arr([rv])), "sp_table_bind_top with " + what)
        for k, (t, v) in enumerate(zip(lst, vals)):
            assert len(t) == len(v), (what, k, len(t))
            _same_table("bind", t, v, "table %d after the refused call (%s)" % (k, what))
    _ok(capi.lib.sp_table_bind_top(ctx.h, _handles(tabs), sz(5), _arr([rv])), "sp_table_bind_top after the refusals")
    for k, t in enumerate(tabs):
        assert len(t) == n // 2
        _same_table("bind", t, F.bind(T[k][0], rv), "table %d bound after the refusals" % k)
    _free(tabs + list(extra.values()))


@_flags_device_errors
def test_bind_top_refuses_the_whole_list_or_nothing(ctx):
    """a fifth table of another length (the first four are a launch of their own), a length that is no power of two, a shorter table in
    front: SP_EINVAL, and every table keeps its length and contents"""
    _bind_top_refusals(ctx, [("five tables, the fifth of another length", [0, 1, 2, 3, "odd"]), ("a length of 6", ["six"]),
                             ("a shorter table first", ["odd", 0])])


@_flags_device_errors
def test_bind_top_refuses_a_table_listed_twice(ctx):
    """next to itself, and across two groups of four: it would be bound twice and its length halved twice"""
    _bind_top_refusals(ctx, [("a table listed twice", [0, 0]), ("the first table again as the fifth", [0, 1, 2, 3, 0]),
                             ("the fourth table again as the fifth", [0, 1, 2, 3, 3])])


@pytest.mark.parametrize("ntabs", HEADS_CASES)
@_flags_device_errors
def test_bind_top_heads_up_to_the_result_area(ctx, ntabs):
    """sp_table_bind_top_heads on 1, 256 (one block), 257 and 1024 tables (the 32 KiB result area); with 1024 also the refusals: one table
    more, a table of length 4 in the list, a table listed twice: every table unchanged"""
    from spartan_amd import capi
    L = capi.lib
    pool = F.edge_table("a", 2 * (ntabs + 1), 130)
    vals = [[pool[2 * k], pool[2 * k + 1]] for k in range(ntabs + 1)]
    tabs = [_up(ctx, v) for v in vals]
    r = F.edge_challenges(ntabs)[3 if ntabs != 257 else 2]
    out = (ctypes.c_uint64 * (4 * (ntabs + 1)))()
    if ntabs == HEADS_CASES[-1]:
        four = _up(ctx, F.edge_table("a", 4, 131))
        for what, lst in (("1025 tables", tabs), ("a table of length 4 alone", [four]), ("a table of length 4 among the others", tabs[:5] + [four]),
                          ("a table listed twice", tabs[:7] + [tabs[2]])):
            _refused(L.sp_table_bind_top_heads(ctx.h, _handles(lst), sz(len(lst)), _arr([r]), out), "sp_table_bind_top_heads with " + what)
        assert len(four) == 4
        _same_table("heads", four, F.edge_table("a", 4, 131), "the table of length 4 after the refused call")
        four.free()
        o2 = (ctypes.c_uint64 * (4 * 2 * 512))()      # unchanged: both entries of every table, 512 tables per gather
        for k0 in (0, 512, 513):
            _ok(L.sp_table_gather(ctx.h, _handles(tabs[k0:k0 + 512]), None, sz(512), sz(2), o2), "sp_table_gather")
            _same("heads", _ints(o2, 1024), [x for v in vals[k0:k0 + 512] for x in v], "the tables after the refused calls")
        assert all(len(t) == 2 for t in tabs)
    _ok(L.sp_table_bind_top_heads(ctx.h, _handles(tabs[:ntabs]), sz(ntabs), _arr([r]), out), "sp_table_bind_top_heads ntabs=%d" % ntabs)
    want = [F.bind(v, r)[0] for v in vals[:ntabs]]
    _same("heads", _ints(out, ntabs), want, "sp_table_bind_top_heads ntabs=%d r=%#x" % (ntabs, r))
    assert all(len(t) == 1 for t in tabs[:ntabs]) and len(tabs[ntabs]) == 2
    for k in sorted({0, ntabs // 2, ntabs - 1}):
        _same_table("heads", tabs[k], [want[k]], "table %d after the last round" % k)
    _free(tabs)


@_flags_device_errors
def test_heads_and_gather_at_the_result_area_and_the_capacity(ctx):
    """sp_table_heads / sp_table_gather on index-tagged tables: ntabs x count = 1024 accepted (1024 x 1, 4 x 256), 1025 refused (1025 x 1,
    5 x 205); a window that ends at a table's capacity accepted, one entry further refused"""
    from spartan_amd import capi
    L = capi.lib
    cap = 300
    vals = [F.tagged(cap, k) for k in range(5)]
    tabs = [_up(ctx, v) for v in vals]
    out = (ctypes.c_uint64 * (4 * 1025))()
    offs = [cap - 256, 0, 17, 44, 1]
    _ok(L.sp_table_gather(ctx.h, _handles(tabs[:4]), (sz * 4)(*offs[:4]), sz(4), sz(256), out), "sp_table_gather 4 x 256")
    _same("heads", _ints(out, 1024), F.gather(vals[:4], offs[:4], 256), "sp_table_gather 4 x 256, table 0 read up to its capacity")
    _refused(L.sp_table_gather(ctx.h, _handles(tabs), (sz * 5)(*offs), sz(5), sz(205), out), "sp_table_gather 5 x 205")
    _refused(L.sp_table_gather(ctx.h, _handles(tabs[:4]), (sz * 4)(cap - 255, 0, 17, 44), sz(4), sz(256), out), "sp_table_gather past a capacity")
    _refused(L.sp_table_gather(ctx.h, _handles(tabs[:2]), (sz * 2)(0, cap), sz(2), sz(1), out), "sp_table_gather at off = cap")
    _ok(L.sp_table_gather(ctx.h, _handles(tabs[:2]), (sz * 2)(0, cap - 1), sz(2), sz(1), out), "sp_table_gather of the last entry")
    _same("heads", _ints(out, 2), [vals[0][0], vals[1][cap - 1]], "sp_table_gather of the last entry")
    many_vals = F.tagged(1025, 9)
    many = [_up(ctx, [x]) for x in many_vals]
    _ok(L.sp_table_heads(ctx.h, _handles(many[:1024]), sz(1024), out), "sp_table_heads of 1024 tables")
    _same("heads", _ints(out, 1024), many_vals[:1024], "sp_table_heads of 1024 tables")
    _refused(L.sp_table_heads(ctx.h, _handles(many), sz(1025), out), "sp_table_heads of 1025 tables")
    _free(tabs + many)


# ------------------------------------------------------------------ the copy kernels of the sharding helpers
@pytest.mark.parametrize("n", SPLIT_LENS)
@_flags_device_errors
def test_residue_split_pack_unpack_index_maps(ctx, n):
    """sp_table_residue_split for W in {1, 3, 4, len} and every g (refused where W does not divide the length, and at g = W), sp_tables_pack
    of the sub-tables, sp_tables_unpack_residues back into fresh tables, on distinct index-tagged residues; sp_table_add_into on edge values"""
    from spartan_amd import capi
    L = capi.lib
    nt = 2
    src = [F.tagged(n, 20 + t) for t in range(nt)]
    tsrc = [_up(ctx, v) for v in src]
    for W in sorted({n if w == "len" else w for w in SPLIT_W}):
        h = vp()
        if n % W or W > n:
            _refused(L.sp_table_residue_split(ctx.h, tsrc[0].h, sz(W), sz(0), ctypes.byref(h)), "sp_table_residue_split n=%d W=%d" % (n, W))
            continue
        _refused(L.sp_table_residue_split(ctx.h, tsrc[0].h, sz(W), sz(W), ctypes.byref(h)), "sp_table_residue_split with g = W")
        sub = n // W
        buf = []
        for g in range(W):
            parts = []
            for t in range(nt):
                h = vp()
                _ok(L.sp_table_residue_split(ctx.h, tsrc[t].h, sz(W), sz(g), ctypes.byref(h)), "sp_table_residue_split n=%d W=%d g=%d" % (n, W, g))
                parts.append(capi.Table(ctx, h))
                assert len(parts[-1]) == sub
                if g in (0, 1, W - 1):      # every g goes through the pack below; these also as tables
                    _same_table("copy", parts[-1], F.residue_split(src[t], W, g), "sp_table_residue_split n=%d W=%d g=%d table %d" % (n, W, g, t))
            o = (ctypes.c_uint64 * (4 * nt * sub))()
            _ok(L.sp_tables_pack(ctx.h, _handles(parts), sz(nt), sz(sub), o), "sp_tables_pack n=%d W=%d g=%d" % (n, W, g))
            got = _ints(o, nt * sub)
            _same("copy", got, F.pack([F.residue_split(s, W, g) for s in src], sub), "sp_tables_pack of the residues g=%d, n=%d W=%d" % (g, n, W))
            buf += got
            _free(parts)
        fresh = [capi.Table.alloc(ctx, n) for _ in range(nt)]
        _ok(L.sp_tables_unpack_residues(ctx.h, _handles(fresh), sz(nt), sz(W), sz(sub), _arr(buf)), "sp_tables_unpack_residues n=%d W=%d" % (n, W))
        assert F.unpack_residues(buf, nt, W, sub) == src      # the model's map is the inverse of split and pack
        for t in range(nt):
            assert len(fresh[t]) == n
            _same_table("copy", fresh[t], src[t], "table %d after sp_tables_unpack_residues n=%d W=%d" % (t, n, W))
        _free(fresh)
    (A, ra), (B, rb) = _edge("a", n, 140), _edge("c", n, 141)
    ta, tb = _up(ctx, raw=ra), _up(ctx, raw=rb)
    _ok(L.sp_table_add_into(ctx.h, ta.h, tb.h), "sp_table_add_into n=%d" % n)
    _same_table("copy", ta, [(x + y) % Q for x, y in zip(A, B)], "sp_table_add_into n=%d" % n)
    _same_table("copy", tb, B, "the source of sp_table_add_into")
    _free(tsrc + [ta, tb])
