"""The fixed-base row commitments (sp_commit_rows, sp_commit_rows_dev, _dev_begin, _dev_start, _upload_start, sp_commit_rows_partial,
sp_msm_indexed: spartan_amd/csrc/commit.hip and the lookup forms of msm_rows.hip, msm_queue.hip, msm_lds.hip) on EDGE VALUES, at EVERY BOUNDARY
OF THEIR DISPATCH. tests/test_gpu_kernels.py and tests/msm_forms_worker.py hold hand-picked shapes on random-ish scalars; here every shape sits on
a threshold of msm_plan / msm_launch / msm_enqueue_reduce / msm_q_cut / msm_lds_shape with its neighbour on the other side, and the form that
ran is OBSERVED: tests/commit_reference.plan (which reads the thresholds from the source) says how many launches of each profiling family
(msm_windows_fixed, msm_rows_fixed, msm_reduce_pass, msm_reduce_compress) a call makes, and sp_prof_read says how many it made; for the queue
form sp_prof_read_spans' issued_adds must be 64 x commit_reference.issued_tiles — zero there is a case that did not take the queue form.
(The launch counts tell the lookup form, the throughput forms, the reduction depth and the encode route apart; among the strip, balanced and
LDS forms they do not: those cases rest on the plan, which tests/test_commit_reference.py checks against the source.)

  tree       rows <= 8: P = 256 | 288 partial sums (one | two workgroups per row), 256 | 257 workgroups per row (the strided loop of the row
             reducer), rows 8 | 9, the blind as the column that crosses; encode.device 0 and 1 (fused | three launches)
  line       rows x columns x windows = 2^19 on both sides at 8 and at 9 rows; the few-row strip form with more than 2048 partial sums
  reduce     9 rows: 2040 | 2091 partial sums (one | two passes, a last chunk of 43), every product columns x windows below 300
  encode     rows 63 | 64 (in the reduction | one lane per row) and 1024 | 1025 (result page | staging copy), lookup- and throughput-sized
  strip      msm.form = 3: no xcd order (255, 300 rows), xcd order with idle tiles (1280), two columns per strip with a one-column last
             strip (2048 x 513), the persistent background launch and the plain one (bg.eighths = 0)
  flat       msm.form = 3: runs clamped by units / 4 | by the resident workgroups, runs that do not divide the units, the blind as the last
             column, 1 / 2 / 4 row-blocks, the upload in 4 chunks and in 1
  queue      rows 255 | 256, 257, 320, 321, 65536 | 65600; msm.q_units 4, 5, 32, 4096 (recut, the floor of 4, a clipped last run);
             msm.q_waves 4 | 12; co-resident through dev_begin and through a dev_start that meets it; zero groups, one live row, short scalars
  lds        msm.lds_bits 6 and 10, msm.form = 1: rows 511 | 512, 768 | 769, 960 | 961 (4, 3, 1, 0 loader wavefronts), 1024 | 1025,
             2048 | 2049; the background grid limit
  digits     the digit pool of every geometry (5, 8, 13, 15 bits; 17, 18, 26, 32 windows) through the flat, queue and strip forms, which
             rebuild a carry in the middle of a scalar; the LDS form's at 6 and 10 bits
  positions  g_off at the last legal offset, h_idx below g_off, z_off != 0, sp_commit_rows_partial with z_stride > cols against orc_pt_msm,
             sp_msm_indexed with repeated and descending indices on both sides of its staging boundary
  refusals   every argument check of the seven entry points, each followed by a correct call on the same context

Rows are filled from the digit pool of the set's geometry plus the edge pool, laid out cyclically so that every value occurs. A tall matrix takes
its rows from a pool of 65 (commit_reference.row_pool_matrix): the oracle is asked once per pool row. Every comparison is exact and counted per
section (printed when the module ends). After an unexpected status nothing further is started (the guard of tests/test_gpu_spark_edges.py).
Every option used here is read at the launch (or, msm.wbits / msm.windows / msm.lds_bits, when a set is built), so all of it runs in one
process; no worker is needed.

Found by this module: sp_commit_rows_upload_start with upload.chunks = 1 under the default form plans the queue form and dropped its slot
counts on the way to the reduction, which then added slots no wavefront had written (case w5-1024x12+b-upload-upload_chunks1: all 1024 rows
wrong before the fix in commit.hip).

Not reached here: choose_geom's budgets, the shard paths, the out-of-memory returns; `strip > cols` (more than 2^19 rows; the clamp changes
no launch: tests/test_commit_reference.py), `counts` inside k_pt_reduce_pass and the k = 4.. tail of the LDS form's hooked DMA (unreachable:
the same module)."""
import ctypes, hashlib, random
from collections import namedtuple
import pytest
from tests import commit_reference as CR
from tests.helpers import Q, vp, sz, gens_bytes, mont_bulk
from tests.test_gpu_spark_edges import _DEVICE_ERROR, _ok, _refused
from tests.test_gpu_spark_edges import _nothing_after_a_device_error      # the autouse guard: a fixture of this module too

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ the case lists (imported by tests/test_commit_reference.py: no GPU needed)
# generator sets: name -> (points, msm.wbits, msm.windows, msm.lds_bits); a fresh label per set (a resident table set is reused whatever its width)
SETS = {"w5": (2050, 5, 0, 0), "n32": (40, 0, 32, 0), "dflt": (20, 0, 0, 0), "l6": (40, 5, 0, 6), "l10": (40, 5, 0, 10)}
DEFAULT_WINDOWS = 17      # what the policy gives a small set (gens.hip, choose_geom): asserted when the set is built
DIGIT_GEOMS = [(5, 0), (8, 0), (13, 0), (15, 0), (0, 17), (0, 18), (0, 26), (0, 32)]      # (msm.wbits, msm.windows)
for _w, _n in DIGIT_GEOMS:
    SETS["g_%d_%d" % (_w, _n)] = (34, _w, _n, 0)
POOL = 65      # rows of a row pool: odd, more than a wavefront, coprime to the stride 7

Case = namedtuple("Case", "sec name set rows cols blind role content opts")
# role: host (sp_commit_rows) | sync (sp_commit_rows_dev) | begin | start | upload | start_shared (a dev_start issued while a dev_begin of the same
# shape is uncollected: both are compared). opts: commit_reference.plan's option names.
OPTION_KEYS = {"form": "msm.form", "device_encode": "encode.device", "q_waves": "msm.q_waves", "q_bg_waves": "msm.q_bg_waves", "q_units": "msm.q_units",
               "bg_eighths": "bg.eighths", "upload_chunks": "upload.chunks", "upload_overlap": "upload.overlap"}


def K(sec, set_, rows, cols, blind=0, role="sync", content="pool", **opts):
    name = "%s-%dx%d%s-%s%s%s" % (set_, rows, cols, "+b" if blind else "", role, "" if content == "pool" else "-" + content,
                                  "".join("-%s%d" % kv for kv in sorted(opts.items())))
    return Case(sec, name, set_, rows, cols, blind, role, content, opts)


TREE_CASES = [K("tree", s, r, c, b, role, device_encode=de)
              for de in (0, 1)
              for s, r, c, b, role in [("n32", 1, 8, 0, "host"), ("n32", 1, 8, 1, "host"), ("n32", 1, 9, 0, "sync"), ("n32", 8, 8, 0, "sync"), ("n32", 8, 8, 1, "host"),
                                       ("n32", 9, 8, 0, "host"), ("n32", 9, 8, 1, "sync"),
                                       ("w5", 1, 1285, 0, "host"), ("w5", 1, 1285, 1, "sync"), ("w5", 1, 1286, 0, "sync"),
                                       ("w5", 8, 1142, 0, "sync"), ("w5", 9, 1142, 0, "host")]]
LINE_CASES = [K("line", "w5", r, c, b, role) for r, c, b, role in [(8, 1285, 0, "sync"), (8, 1286, 0, "sync"), (8, 1284, 1, "host"), (8, 1285, 1, "host"),
                                                                   (9, 1142, 0, "sync"), (9, 1143, 0, "host"), (9, 1141, 1, "sync"), (9, 1142, 1, "sync"), (8, 2049, 0, "sync")]]
LINE_CASES += [K("line", "w5", 8, 1286, 0, "sync", device_encode=1)]      # the few-row strip form with every encode on the device
REDUCE_CASES = [K("reduce", "w5", 9, 40, 0), K("reduce", "w5", 9, 41, 0), K("reduce", "w5", 9, 40, 1, "host"), K("reduce", "w5", 9, 39, 1)]
SMALL_P_CASES = [K("reduce", s, 9, c - b, b, "host" if c % 2 else "sync") for s, nwin in (("w5", 51), ("n32", 32), ("dflt", DEFAULT_WINDOWS))
                 for c in range(1, 300 // nwin + 1) for b in ((0, 1) if c > 1 else (0,)) if c * nwin < 300]
ENCODE_CASES = [K("encode", "w5", r, c, 1, role) for r in (63, 64, 1024, 1025) for c, role in ((3, "host"), (170 if r < 256 else 12, "sync"))]
ENCODE_CASES += [K("encode", "w5", r, 170, 0, "start") for r in (63, 64)]
STRIP_CASES = [K("strip", "w5", 255, 41, 0, form=3), K("strip", "w5", 300, 41, 1, form=3), K("strip", "w5", 1280, 11, 0, form=3), K("strip", "w5", 1280, 16, 1, "host", form=3),
               K("strip", "w5", 2048, 513, 0, form=3), K("strip", "w5", 300, 41, 0, "begin", form=3), K("strip", "w5", 1280, 11, 0, "begin", form=3),
               K("strip", "w5", 300, 41, 0, "begin", form=3, bg_eighths=0), K("strip", "w5", 300, 41, 1, "start_shared", form=3), K("strip", "w5", 256, 41, 1, "start_shared", form=3)]
FLAT_CASES = [K("flat", "w5", 256, 40, 1, form=3), K("flat", "w5", 256, 41, 0, form=3), K("flat", "w5", 256, 61, 0, form=3), K("flat", "w5", 256, 72, 0, form=3),
              K("flat", "w5", 256, 71, 1, "host", form=3), K("flat", "w5", 512, 21, 1, form=3), K("flat", "w5", 1024, 12, 1, form=3), K("flat", "w5", 1280, 12, 1, form=3),
              K("flat", "w5", 1024, 12, 1, "upload", form=3), K("flat", "w5", 1024, 12, 0, "upload", form=3, upload_chunks=1), K("flat", "w5", 1024, 12, 1, "upload"),
              K("flat", "w5", 1024, 12, 1, "upload", form=3, upload_overlap=0), K("flat", "w5", 1000, 12, 1, "upload", form=3), K("flat", "w5", 256, 41, 1, "start", form=3)]
QUEUE_CASES = [K("queue", "w5", r, 41, 1) for r in (255, 256, 257, 320, 321)]
QUEUE_CASES += [K("queue", "w5", 256, 41, 1, q_units=u, q_waves=4) for u in (4, 5, 32, 4096)]
QUEUE_CASES += [K("queue", "w5", 256, 41, 1, q_units=u) for u in (4, 5)] + [K("queue", "w5", 256, 46, 0), K("queue", "w5", 1024, 41, 1, q_waves=4), K("queue", "w5", 1024, 41, 1, q_waves=4, q_units=4)]
QUEUE_CASES += [K("queue", "w5", 65536, 1, 1, "host"), K("queue", "w5", 65600, 1, 1, "host")]
QUEUE_CASES += [K("queue", "w5", 256, 41, 0, "begin"), K("queue", "w5", 320, 41, 1, "start_shared"), K("queue", "w5", 256, 41, 1, "start"), K("queue", "w5", 1024, 12, 1, "upload", upload_chunks=1)]
QUEUE_CASES += [K("queue", "w5", 321, 41, 1, "sync", content) for content in ("zero_groups", "short")] + [K("queue", "w5", 320, 41, 0, "begin", "zero_groups"), K("queue", "w5", 256, 41, 1, "sync", "short", q_units=4)]
LDS_CASES = [K("lds", s, r, 21, 1, form=1) for s in ("l6", "l10") for r in (511, 512, 768, 769, 960, 961, 1024, 1025, 2048, 2049)]
LDS_CASES += [K("lds", s, 40000, 1, 0, "begin", form=1, bg_eighths=1) for s in ("l6", "l10")]
LDS_CASES += [K("lds", "l10", 1024, 21, 0, "begin", form=1), K("lds", "l10", 769, 21, 1, "start_shared", form=1), K("lds", "l6", 2048, 21, 1, "upload", form=1), K("lds", "l10", 512, 1, 1, form=1)]


def digit_cols(nwin):
    """columns + blind so that 1000 rows are past the lookup form: the flat, queue and strip forms take the shape"""
    return -(-((1 << 19) // 1000 + 1) // nwin)


DIGIT_CASES = []
for _w, _n in DIGIT_GEOMS:
    _s = "g_%d_%d" % (_w, _n)
    _c = digit_cols(CR.Geom(wbits=_w, windows=_n).nwin) - 1
    DIGIT_CASES += [K("digits", _s, 1024, _c, 1, "sync", "digits", form=3), K("digits", _s, 1024, _c, 1, "sync", "digits", q_units=4), K("digits", _s, 1000, _c, 1, "sync", "digits", form=3)]
DIGIT_CASES += [K("digits", s, 1024, 21, 1, "sync", "digits", form=1) for s in ("l6", "l10")]
POSITION_ROWS = [2, 9, 256]      # tree | lookup | queue at 41 columns of the 5-bit set
INDEXED_CASES = [(1, 625), (1, 626), (2, 331), (2, 332), (8, 86), (8, 87), (9, 77), (9, 78)]      # (rows, cols): the host-mapped page | the staging buffer
ALL_CASES = TREE_CASES + LINE_CASES + REDUCE_CASES + SMALL_P_CASES + ENCODE_CASES + STRIP_CASES + FLAT_CASES + QUEUE_CASES + LDS_CASES + DIGIT_CASES

COUNTS = {k: 0 for k in ("tree", "line", "reduce", "encode", "strip", "flat", "queue", "lds", "digits", "positions", "refusals")}      # exact comparisons per section


def geom_of(name, windows=DEFAULT_WINDOWS):
    _, w, nw, _ = SETS[name]
    return CR.Geom(wbits=w, windows=nw if (w or nw) else windows)


def lds_geom_of(name):
    return CR.Geom(wbits=SETS[name][3]) if SETS[name][3] else None


def plan_role(role):
    return {"host": "sync", "start_shared": "start"}.get(role, role)


def plans_of(case, n_cus, flat_slots, nwin=None):
    """the plans of the launches a case makes, in issue order: one, or (start_shared) the background commit and the foreground one that meets it"""
    ge, gl = geom_of(case.set), lds_geom_of(case.set)
    nwin = nwin or ge.nwin
    mk = lambda role, blind, **kw: CR.plan(case.rows, case.cols, blind, nwin, dict(case.opts, **kw), n_cus, flat_slots, gl.nwin if gl else None, role)
    if case.role == "start_shared":
        return [mk("begin", 0), mk("start", case.blind, shares_chip=True)]
    return [mk(plan_role(case.role), case.blind)]


def _seed(*parts):
    return int.from_bytes(hashlib.sha256(repr(parts).encode()).digest()[:8], "little")


def value_pool(set_):
    ge, gl = geom_of(set_), lds_geom_of(set_)
    return CR.digit_pool(ge) + (CR.digit_pool(gl) if gl else []) + CR.edge_pool()


def pool_rows(set_, cols, content, npool):
    """(rows of the pool, their blinds): every value of the set's value pool in turn (each row begins three values further on, so a column sees
    them all); short: scalars of 1, 7 and 33 bits"""
    if content == "short":
        rng = random.Random(_seed("short", set_, cols))
        draw = lambda: rng.getrandbits(rng.choice((1, 7, 33)))
        return [[draw() for _ in range(cols)] for _ in range(npool)], [draw() for _ in range(npool)]
    vals = value_pool(set_)
    return [[vals[(r * cols + j + 3 * r) % len(vals)] for j in range(cols)] for r in range(npool)], [vals[(5 * r + 1) % len(vals)] for r in range(npool)]


_MATRICES = {}


def matrix_of(case):
    """(pool rows, pool blinds, idx): row r of the case's matrix is pool row idx[r]; one more pool row, the last, is all zero (blind 0)"""
    key = (case.set, case.rows, case.cols, case.content)
    if key not in _MATRICES:
        npool = min(case.rows, POOL)
        rows_, blinds = pool_rows(case.set, case.cols, case.content, npool)
        idx = list(range(case.rows)) if case.rows <= POOL else CR.row_pool_matrix(rows_, case.rows)[1]
        zero = len(rows_)
        if case.content == "zero_groups":      # whole wavefronts of zero rows next to live ones; group 2 holds one live row
            idx = [zero if ((r // 64) % 2 == 1 or (r // 64 == 2 and r % 64 != 37)) else i for r, i in enumerate(idx)]
        _MATRICES.clear()      # (one matrix at a time: the cases of a shape follow each other)
        _MATRICES[key] = (rows_ + [[0] * case.cols], blinds + [0], idx)
    return _MATRICES[key]


def flat_matrix(case):
    """(Z, blinds) as canonical integers, row-major"""
    rows_, blinds, idx = matrix_of(case)
    return [x for i in idx for x in rows_[i]], [blinds[i] for i in idx]


# ------------------------------------------------------------------ the device side
@pytest.fixture(scope="module")
def ctx():
    from spartan_amd import capi
    if _DEVICE_ERROR:
        pytest.fail("not started: an earlier call failed on the device: %s" % _DEVICE_ERROR[0])
    c = capi.Ctx(0)
    c.prof_enable(True)
    yield c
    c.close()
    print("\nexact comparisons per section: %s; total %d" % (", ".join("%s %d" % kv for kv in sorted(COUNTS.items())), sum(COUNTS.values())))


def cu_count():
    """compute units of the first GPU: the KFD topology's simd_count / simd_per_cu of the first node that has any; where that is not
    readable, what a child process with torch reports (a second HIP runtime in this process finds no device once the library holds it)"""
    import glob, subprocess, sys
    for f in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"), key=lambda x: int(x.split("/")[-2])):
        try:
            kv = dict(l.split()[:2] for l in open(f).read().splitlines() if len(l.split()) >= 2)
        except OSError:
            continue
        if int(kv.get("simd_count", 0)) and int(kv.get("simd_per_cu", 0)):
            return int(kv["simd_count"]) // int(kv["simd_per_cu"])
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@pytest.fixture(scope="module")
def chip():
    """(CUs, resident workgroups of the balanced form as the plan assumes them: commit_reference reads the per-CU figure msm_flat_slots falls back to)"""
    n = cu_count()
    assert n in (128, 256, 304) or n > 0, n
    print("\n%d compute units" % n)
    return n, CR.constants()["FLAT_PER_CU"] * n


@pytest.fixture(scope="module")
def gsets(ctx, orc):
    """name -> (Gens, [compressed points]) of SETS, built on first use with the set's own window geometry"""
    from spartan_amd import capi
    built = {}

    def get(name):
        if name in built:
            return built[name]
        n, wbits, windows, lds_bits = SETS[name]
        label = b"gens_commit_edges_" + name.encode()
        ctx.set_option("msm.wbits", wbits); ctx.set_option("msm.windows", windows); ctx.set_option("msm.lds_bits", lds_bits)      # read when a generator set is built
        try:
            g = capi.Gens(ctx, compressed=gens_bytes(orc, n - 1, label))
        finally:
            ctx.set_option("msm.wbits", 0); ctx.set_option("msm.windows", 0); ctx.set_option("msm.lds_bits", 0)
        ge = geom_of(name)
        assert g.windows() == ge.nwin and g.window_bits() == ge.wbits, (name, g.windows(), g.window_bits())
        gl = lds_geom_of(name)      # (the LDS form's packed tables: 96-byte entries)
        assert capi.lib.sp_gens_table_bytes(g.h) == ge.table_bytes(n) + (n * gl.pt_entries * 96 if gl else 0), name
        built[name] = (g, [g.compressed[32 * i:32 * i + 32] for i in range(n)])
        return built[name]
    yield get
    for g, _ in built.values():
        g.free()


class _Options:
    """options for the length of a with-block: unlocked, set, and restored in any case (keys: commit_reference.plan's names)"""
    def __init__(self, ctx, opts):
        self.ctx, self.kv = ctx, {OPTION_KEYS[k]: v for k, v in opts.items()}

    def __enter__(self):
        self.ctx.set_option("testing.unlock", 1)
        self.old = {k: self.ctx.get_option(k) for k in self.kv}
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)
        self.ctx.set_option("testing.unlock", 0)


def _eq(sec, got, want, what):
    if got != want:
        n = len(want) // 32
        bad = [r for r in range(n) if got[32 * r:32 * r + 32] != want[32 * r:32 * r + 32]]
        pytest.fail("%s: %d of %d rows differ, first %s" % (what, len(bad), n, bad[:8]))
    COUNTS[sec] += len(want) // 32


_POOL_COMMITS = {}


def expected_of(orc, P, case, g_off=0, h_idx=None):
    """(with blinds, without): the pool's commitments are computed once per (set, columns, content, position) and shared"""
    rows_, blinds, idx = matrix_of(case)
    h_idx = SETS[case.set][0] - 1 if h_idx is None else h_idx
    key = (case.set, case.cols, case.content, len(rows_), g_off, h_idx, bool(case.blind))
    if key not in _POOL_COMMITS:
        G, H = b"".join(P[g_off:g_off + case.cols]), P[h_idx]
        ident = list(range(len(rows_)))
        _POOL_COMMITS[key] = (CR.expected(orc, G, H, rows_, ident, blinds) if case.blind else None, CR.expected(orc, G, H, rows_, ident))
        assert _POOL_COMMITS[key][1][-32:] == CR.NEUTRAL
    wb, wn = _POOL_COMMITS[key]
    pick = lambda w: b"".join(w[32 * i:32 * i + 32] for i in idx)
    return (pick(wb) if wb is not None else None), pick(wn)


FAMILIES = {"windows": "msm_windows_fixed", "rows": "msm_rows_fixed", "reduce_pass": "msm_reduce_pass", "reduce": "msm_reduce_compress"}


def read_issued(ctx):
    from spartan_amd import capi
    cap = 16
    iss = (ctypes.c_double * cap)()
    k = capi.lib.sp_prof_read_spans(ctx.h, FAMILIES["rows"].encode(), None, None, None, iss, ctypes.c_int(cap))
    assert 0 <= k <= cap, k
    return sorted(int(iss[i]) for i in range(k))


def wait(job, rows, what):
    from spartan_amd import capi
    out = (ctypes.c_uint8 * (32 * rows))()
    _ok(capi.lib.sp_job_wait(job, out), "sp_job_wait " + what)
    return bytes(out)


def run_case(ctx, orc, gsets, chip, case):
    """one case: the call(s) of its role, each result against the oracle, then the launches observed against the plan"""
    from spartan_amd import capi
    L = capi.lib
    g, P = gsets(case.set)
    rows, cols = case.rows, case.cols
    plans = plans_of(case, chip[0], chip[1], g.windows())
    h_idx = SETS[case.set][0] - 1
    want_b, want_n = expected_of(orc, P, case)
    Z, bl = flat_matrix(case)
    Zm, blm = mont_bulk(Z), (mont_bulk(bl) if case.blind else None)
    what = case.name
    with _Options(ctx, case.opts):
        ctx.prof_reset()
        if case.role == "host":
            out = (ctypes.c_uint8 * (32 * rows))()
            _ok(L.sp_commit_rows(ctx.h, g.h, sz(0), sz(h_idx), Zm, sz(rows), sz(cols), blm, out), "sp_commit_rows " + what)
            _eq(case.sec, bytes(out), want_b if case.blind else want_n, what)
        elif case.role == "upload":
            t = capi.Table.alloc(ctx, rows * cols)
            _ok(L.sp_ctx_sync(ctx.h), "sp_ctx_sync")
            ctx.prof_reset()
            job = vp()
            _ok(L.sp_commit_rows_upload_start(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), Zm, sz(rows), sz(cols), blm, ctypes.byref(job)), "sp_commit_rows_upload_start " + what)
            _eq(case.sec, wait(job, rows, what), want_b if case.blind else want_n, what)
            assert bytes(t.download()) == bytes(Zm), what      # the rows are left in the table
            t.free()
        else:
            t = capi.Table.upload(ctx, Zm, rows * cols)
            _ok(L.sp_ctx_sync(ctx.h), "sp_ctx_sync")
            ctx.prof_reset()
            if case.role == "sync":
                out = (ctypes.c_uint8 * (32 * rows))()
                _ok(L.sp_commit_rows_dev(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), sz(rows), sz(cols), blm, out), "sp_commit_rows_dev " + what)
                _eq(case.sec, bytes(out), want_b if case.blind else want_n, what)
            else:
                bg, fg = vp(), vp()
                if case.role in ("begin", "start_shared"):
                    _ok(L.sp_commit_rows_dev_begin(ctx.h, g.h, sz(0), t.h, sz(0), sz(rows), sz(cols), ctypes.byref(bg)), "sp_commit_rows_dev_begin " + what)
                if case.role in ("start", "start_shared"):      # (start_shared: queued while the background job is uncollected)
                    _ok(L.sp_commit_rows_dev_start(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), sz(rows), sz(cols), blm, ctypes.byref(fg)), "sp_commit_rows_dev_start " + what)
                    _eq(case.sec, wait(fg, rows, what), want_b if case.blind else want_n, what + " (dev_start)")
                if bg:
                    _eq(case.sec, wait(bg, rows, what), want_n, what + " (dev_begin)")
            t.free()
        prof = ctx.prof_read()
        issued = read_issued(ctx)
    seen = {k: prof.get(f, {"launches": 0})["launches"] for k, f in FAMILIES.items()}
    planned = {k: sum(p["launches"][k] for p in plans) for k in FAMILIES}
    assert seen == planned, (what, "launches per family", seen, planned, [p["form"] for p in plans])
    ge = geom_of(case.set, g.windows())
    tiles = sorted(64 * CR.issued_tiles(Z, rows, cols, bl if p["ncol"] > cols else None, ge, p["len"]) for p in plans if p["form"] == "queue")
    assert [x for x in issued if x] == tiles and (not tiles or min(tiles) > 0), (what, "mixed additions issued by the queue form", issued, tiles, [p["form"] for p in plans])
    return plans


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------ 1..9: one case, one call, one plan
@pytest.mark.parametrize("case", TREE_CASES, ids=_ids(TREE_CASES))
def test_lookup_tree_at_one_and_two_workgroups_and_at_the_row_reducer_stride(ctx, orc, gsets, chip, case):
    p, = run_case(ctx, orc, gsets, chip, case)
    assert p["form"] in ("tree1", "tree_fused", "tree_unfused", "windows")


@pytest.mark.parametrize("case", LINE_CASES, ids=_ids(LINE_CASES))
def test_both_sides_of_the_line_between_lookup_and_throughput_forms(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


@pytest.mark.parametrize("case", REDUCE_CASES, ids=_ids(REDUCE_CASES))
def test_one_and_two_reduction_passes(ctx, orc, gsets, chip, case):
    p, = run_case(ctx, orc, gsets, chip, case)
    assert p["form"] == "windows"


@pytest.mark.parametrize("set_", ["w5", "n32", "dflt"])
def test_every_partial_sum_count_below_300(ctx, orc, gsets, chip, set_):
    """k_msm_reduce's pt10_tree_quad on every count columns x windows the geometries give below 300 (non-powers of two)"""
    for case in SMALL_P_CASES:
        if case.set == set_:
            p, = run_case(ctx, orc, gsets, chip, case)
            assert p["form"] == "windows" and p["P"] < 300 and p["encode"] == "in_reduce"


@pytest.mark.parametrize("case", ENCODE_CASES, ids=_ids(ENCODE_CASES))
def test_encode_routes_and_the_result_page(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


@pytest.mark.parametrize("case", STRIP_CASES, ids=_ids(STRIP_CASES))
def test_strip_form(ctx, orc, gsets, chip, case):
    for p in run_case(ctx, orc, gsets, chip, case):
        assert p["form"] in ("strip", "strip_bg")


@pytest.mark.parametrize("case", FLAT_CASES, ids=_ids(FLAT_CASES))
def test_balanced_form(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


@pytest.mark.parametrize("case", QUEUE_CASES, ids=_ids(QUEUE_CASES))
def test_queue_form(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


@pytest.mark.parametrize("case", LDS_CASES, ids=_ids(LDS_CASES))
def test_lds_form(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


@pytest.mark.parametrize("case", DIGIT_CASES, ids=_ids(DIGIT_CASES))
def test_signed_digits_of_the_forms_that_start_inside_a_scalar(ctx, orc, gsets, chip, case):
    run_case(ctx, orc, gsets, chip, case)


# ------------------------------------------------------------------ 10. positions
@pytest.mark.parametrize("rows", POSITION_ROWS)
def test_generator_and_table_positions(ctx, orc, gsets, rows):
    """g_off at the last legal offset, the blind's generator below it, the matrix at an offset of its table"""
    from spartan_amd import capi
    L = capi.lib
    g, P = gsets("w5")
    n, cols, z_off = SETS["w5"][0], 41, 77
    case = K("positions", "w5", rows, cols, 1)
    g_off, h_idx = n - cols, 3
    want_b, want_n = expected_of(orc, P, case, g_off, h_idx)
    Z, bl = flat_matrix(case)
    t = capi.Table.upload(ctx, mont_bulk([Q - 1] * z_off + Z + [Q - 1] * 5), z_off + rows * cols + 5)
    out = (ctypes.c_uint8 * (32 * rows))()
    _ok(L.sp_commit_rows_dev(ctx.h, g.h, sz(g_off), sz(h_idx), t.h, sz(z_off), sz(rows), sz(cols), mont_bulk(bl), out), "sp_commit_rows_dev at g_off = n - cols")
    _eq("positions", bytes(out), want_b, "g_off last, h below, z_off, %d rows" % rows)
    _refused(L.sp_commit_rows_dev(ctx.h, g.h, sz(g_off + 1), sz(h_idx), t.h, sz(z_off), sz(rows), sz(cols), None, out), "g_off one past the last offset")
    if rows > 8:
        bg, fg = vp(), vp()
        _ok(L.sp_commit_rows_dev_begin(ctx.h, g.h, sz(g_off), t.h, sz(z_off), sz(rows), sz(cols), ctypes.byref(bg)), "sp_commit_rows_dev_begin at z_off")
        _ok(L.sp_commit_rows_dev_start(ctx.h, g.h, sz(g_off), sz(h_idx), t.h, sz(z_off), sz(rows), sz(cols), mont_bulk(bl), ctypes.byref(fg)), "sp_commit_rows_dev_start at z_off")
        _eq("positions", wait(fg, rows, "positions"), want_b, "dev_start at z_off, %d rows" % rows)
        _eq("positions", wait(bg, rows, "positions"), want_n, "dev_begin at z_off, %d rows" % rows)
    t.free()


@pytest.mark.parametrize("rows,cols,stride", [(1, 9, 9), (3, 9, 11), (8, 1285, 1290), (8, 1286, 1286), (5, 2049, 2050)])
def test_partial_commitments_with_a_row_stride(ctx, orc, gsets, rows, cols, stride):
    """sp_commit_rows_partial (rows left as points, z_stride >= cols, no blind): tree, fused tree and the few-row strip form. The points are
    encoded on the host (sp_host_points_sum_encode over one set) and compared with orc_pt_msm over the row's scalars."""
    from spartan_amd import capi
    from tests.ipa_reference import _msm
    L = capi.lib
    g, P = gsets("w5")
    g_off, z_off = 1, 3
    vals = value_pool("w5")
    M = [vals[(7 * i + 2) % len(vals)] for i in range(z_off + rows * stride)]      # the gaps between the rows hold values too
    t = capi.Table.upload(ctx, mont_bulk(M), len(M))
    pts = (ctypes.c_uint64 * (16 * rows))()
    _ok(L.sp_commit_rows_partial(ctx.h, g.h, sz(g_off), t.h, sz(z_off), sz(stride), sz(rows), sz(cols), pts), "sp_commit_rows_partial")
    out = (ctypes.c_uint8 * (32 * rows))()
    _ok(L.sp_host_points_sum_encode(pts, sz(1), sz(rows), out), "sp_host_points_sum_encode")
    want = b"".join(_msm(orc, M[z_off + r * stride:z_off + r * stride + cols], P[g_off:g_off + cols]) for r in range(rows))
    _eq("positions", bytes(out), want, "partial %dx%d stride %d" % (rows, cols, stride))
    t.free()


@pytest.mark.parametrize("rows,cols", INDEXED_CASES)
def test_indexed_commitments_on_both_sides_of_the_staging_boundary(ctx, orc, gsets, rows, cols):
    """sp_msm_indexed: scalars and indices in the host-mapped page | in the device staging buffer; indices descending, with repeats, the
    last generator of the set among them (one index list for all rows)"""
    from tests.ipa_reference import _msm
    g, P = gsets("w5")
    n = SETS["w5"][0]
    idx = [n - 1 - (j // 2) * 3 % n for j in range(cols)]      # descending, every index twice
    idx[-1] = n - 1
    assert any(a > b for a, b in zip(idx, idx[1:])) and len(set(idx)) < len(idx) and max(idx) == n - 1
    vals = value_pool("w5")
    S = [vals[(11 * i + 5) % len(vals)] for i in range(rows * cols)]
    got = g.msm_indexed(idx, mont_bulk(S), rows)
    want = b"".join(_msm(orc, S[r * cols:(r + 1) * cols], [P[j] for j in idx]) for r in range(rows))
    _eq("positions", got, want, "indexed %dx%d staged in the %s" % (rows, cols, "page" if CR.indexed_staging(rows, cols) else "buffer"))


# ------------------------------------------------------------------ what every plan's call leaves behind
# the smallest shape of every plan (all from the lists above), sp_commit_rows_partial at 2 rows and sp_msm_indexed on both sides of its staging boundary
RECORD_CASES = [K("tree", "n32", 1, 8, 0, "host"), K("tree", "n32", 1, 9, 0, "sync"), K("tree", "n32", 1, 9, 0, "sync", device_encode=1),
                K("reduce", "w5", 9, 40, 0), K("reduce", "w5", 9, 41, 0), K("line", "w5", 8, 1286, 0, "sync"),
                K("queue", "w5", 256, 41, 1), K("queue", "w5", 256, 41, 0, "begin"), K("queue", "w5", 256, 41, 1, "start"), K("queue", "w5", 256, 41, 1, "start_shared"),
                K("flat", "w5", 1024, 12, 1, "upload"), K("queue", "w5", 1024, 12, 1, "upload", upload_chunks=1)]
RECORD_PARTIAL = (2, 9, 11)      # rows, cols, z_stride
RECORD_INDEXED = [(1, 625), (1, 626)]
# call -> (round trips by sp_ctx_trips: of a synchronous call its own; of a job those of its start and of its sp_job_wait (start_shared: begin, start,
# wait of the foreground job, wait of the background job), {profile family: (records, algorithmic bytes)} of every family the call left a record in).
# MEASURED, not derived from the code under test: this test printed the table on the library as it stood before the row commitments were given one
# plan and one launch path (256 compute units), and it was written down here as literals. The calls must go on leaving exactly this behind.
COMMIT_RECORDS = {
    'n32-1x8-host': ((1,), {'msm_windows_fixed': (1, 416.0)}),
    'n32-1x9-sync': ((1,), {'msm_windows_fixed': (1, 608.0)}),
    'n32-1x9-sync-device_encode1': ((1,), {'msm_windows_fixed': (1, 608.0), 'msm_reduce_compress': (2, 608.0)}),
    'w5-9x40-sync': ((1,), {'msm_windows_fixed': (1, 2361600.0), 'msm_reduce_compress': (1, 2350368.0)}),
    'w5-9x41-sync': ((1,), {'msm_windows_fixed': (1, 2420640.0), 'msm_reduce_pass': (1, 2413152.0), 'msm_reduce_compress': (1, 4608.0)}),
    'w5-8x1286-sync': ((1,), {'msm_rows_fixed': (1, 329472.0), 'msm_reduce_compress': (1, 1317120.0)}),
    'w5-256x41+b-sync': ((1,), {'msm_rows_fixed': (1, 344064.0), 'msm_reduce_compress': (2, 27312128.0)}),
    'w5-256x41-begin': ((0, 0), {'msm_rows_fixed': (1, 344064.0), 'msm_reduce_compress': (2, 18923520.0)}),
    'w5-256x41+b-start': ((0, 0), {'msm_rows_fixed': (1, 344064.0), 'msm_reduce_compress': (2, 27312128.0)}),
    'w5-256x41+b-start_shared': ((0, 0, 0, 0), {'msm_rows_fixed': (2, 688128.0), 'msm_reduce_compress': (4, 37847040.0)}),
    'w5-1024x12+b-upload': ((0, 0), {'msm_rows_fixed': (4, 425984.0), 'msm_reduce_compress': (2, 21823488.0)}),
    'w5-1024x12+b-upload-upload_chunks1': ((0, 0), {'msm_rows_fixed': (1, 425984.0), 'msm_reduce_compress': (2, 33751040.0)}),
    'partial-2x9': ((1,), {'msm_windows_fixed': (1, 1216.0)}),
    'indexed-1x625': ((1,), {'msm_windows_fixed': (1, 40000.0)}),
    'indexed-1x626': ((1,), {'msm_windows_fixed': (1, 40032.0)}),
}


def test_records_and_round_trips_of_every_plan(ctx, orc, gsets):
    """one call of every plan of msm_launch and of the job entry points, sp_commit_rows_partial and sp_msm_indexed: each result against the oracle,
    the round trips each call makes and the profile records it leaves (how many per family, and their algorithmic bytes) are those of COMMIT_RECORDS"""
    from spartan_amd import capi
    from tests.ipa_reference import _msm
    L = capi.lib
    got = {}
    trips = []
    tick = lambda: trips.append(L.sp_ctx_trips(ctx.h))

    def begin():
        ctx.prof_reset()
        del trips[:]
        tick()

    def end(key):
        rec = {n: (v["launches"], v["alg_bytes"]) for n, v in ctx.prof_read().items() if v["launches"] or v["alg_bytes"]}
        got[key] = (tuple(b - a for a, b in zip(trips, trips[1:])), rec)
    for case in RECORD_CASES:
        g, P = gsets(case.set)
        rows, cols, what = case.rows, case.cols, case.name
        h_idx = SETS[case.set][0] - 1
        want_b, want_n = expected_of(orc, P, case)
        want = want_b if case.blind else want_n
        Z, bl = flat_matrix(case)
        Zm, blm = mont_bulk(Z), (mont_bulk(bl) if case.blind else None)
        out, bg, fg = (ctypes.c_uint8 * (32 * rows))(), vp(), vp()
        with _Options(ctx, case.opts):
            t = capi.Table.alloc(ctx, rows * cols) if case.role == "upload" else capi.Table.upload(ctx, Zm, rows * cols)
            _ok(L.sp_ctx_sync(ctx.h), "sp_ctx_sync")
            begin()
            if case.role == "host":
                _ok(L.sp_commit_rows(ctx.h, g.h, sz(0), sz(h_idx), Zm, sz(rows), sz(cols), blm, out), "sp_commit_rows " + what)
            elif case.role == "sync":
                _ok(L.sp_commit_rows_dev(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), sz(rows), sz(cols), blm, out), "sp_commit_rows_dev " + what)
            elif case.role == "upload":
                _ok(L.sp_commit_rows_upload_start(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), Zm, sz(rows), sz(cols), blm, ctypes.byref(fg)), "sp_commit_rows_upload_start " + what)
            if case.role in ("host", "sync", "upload"):
                tick()
            if case.role in ("begin", "start_shared"):
                _ok(L.sp_commit_rows_dev_begin(ctx.h, g.h, sz(0), t.h, sz(0), sz(rows), sz(cols), ctypes.byref(bg)), "sp_commit_rows_dev_begin " + what)
                tick()
            if case.role in ("start", "start_shared"):
                _ok(L.sp_commit_rows_dev_start(ctx.h, g.h, sz(0), sz(h_idx), t.h, sz(0), sz(rows), sz(cols), blm, ctypes.byref(fg)), "sp_commit_rows_dev_start " + what)
                tick()
            if case.role in ("host", "sync"):
                _eq(case.sec, bytes(out), want, what)
            if fg:
                res = wait(fg, rows, what)
                tick()
                _eq(case.sec, res, want, what)
            if bg:
                res = wait(bg, rows, what)
                tick()
                _eq(case.sec, res, want_n, what + " (dev_begin)")
            end(what)
            t.free()
    g, P = gsets("w5")
    vals = value_pool("w5")
    rows, cols, stride = RECORD_PARTIAL
    M = [vals[(7 * i + 2) % len(vals)] for i in range(3 + rows * stride)]
    t = capi.Table.upload(ctx, mont_bulk(M), len(M))
    pts, out = (ctypes.c_uint64 * (16 * rows))(), (ctypes.c_uint8 * (32 * rows))()
    _ok(L.sp_ctx_sync(ctx.h), "sp_ctx_sync")
    begin()
    _ok(L.sp_commit_rows_partial(ctx.h, g.h, sz(1), t.h, sz(3), sz(stride), sz(rows), sz(cols), pts), "sp_commit_rows_partial")
    tick()
    end("partial-%dx%d" % (rows, cols))
    _ok(L.sp_host_points_sum_encode(pts, sz(1), sz(rows), out), "sp_host_points_sum_encode")
    _eq("positions", bytes(out), b"".join(_msm(orc, M[3 + r * stride:3 + r * stride + cols], P[1:1 + cols]) for r in range(rows)), "partial %dx%d" % (rows, cols))
    t.free()
    for rows, cols in RECORD_INDEXED:
        idx = [(5 * j + 1) % SETS["w5"][0] for j in range(cols)]
        S = [vals[(11 * i + 5) % len(vals)] for i in range(rows * cols)]
        Sm = mont_bulk(S)
        begin()
        res = g.msm_indexed(idx, Sm, rows)
        tick()
        end("indexed-%dx%d" % (rows, cols))
        _eq("positions", res, b"".join(_msm(orc, S[r * cols:(r + 1) * cols], [P[j] for j in idx]) for r in range(rows)), "indexed %dx%d" % (rows, cols))
    assert got == COMMIT_RECORDS, "".join("\n    %r: %r," % kv for kv in got.items() if COMMIT_RECORDS.get(kv[0]) != kv[1])


# ------------------------------------------------------------------ 11. refusals
def test_refusals_change_nothing(ctx, orc, gsets):
    """every argument check of the seven entry points returns SP_EINVAL before anything is launched; a correct call on the same context follows
    each entry point's refusals and still matches"""
    from spartan_amd import capi
    L = capi.lib
    g, P = gsets("n32")
    n, rows, cols = SETS["n32"][0], 9, 8
    case = K("refusals", "n32", rows, cols, 1)
    want_b, want_n = expected_of(orc, P, case)
    Z, bl = flat_matrix(case)
    Zm, blm = mont_bulk(Z), mont_bulk(bl)
    t = capi.Table.upload(ctx, Zm, rows * cols)
    out = (ctypes.c_uint8 * (32 * rows))(*([0xA5] * (32 * rows)))
    untouched = bytes([0xA5] * (32 * rows))
    job = vp()
    jr = ctypes.byref(job)
    h = n - 1
    c_, g_, t_ = ctx.h, g.h, t.h

    def refuse(entry, checks):
        for what, rc in checks:
            _refused(rc, "%s, %s" % (entry, what))
            assert bytes(out) == untouched and not job.value, (entry, what)
            COUNTS["refusals"] += 1
    refuse("sp_commit_rows", [
        ("null context", L.sp_commit_rows(None, g_, sz(0), sz(h), Zm, sz(rows), sz(cols), blm, out)), ("null generators", L.sp_commit_rows(c_, None, sz(0), sz(h), Zm, sz(rows), sz(cols), blm, out)),
        ("null Z", L.sp_commit_rows(c_, g_, sz(0), sz(h), None, sz(rows), sz(cols), blm, out)), ("null out", L.sp_commit_rows(c_, g_, sz(0), sz(h), Zm, sz(rows), sz(cols), blm, None)),
        ("no rows", L.sp_commit_rows(c_, g_, sz(0), sz(h), Zm, sz(0), sz(cols), blm, out)), ("no columns", L.sp_commit_rows(c_, g_, sz(0), sz(h), Zm, sz(rows), sz(0), blm, out)),
        ("g_off + cols > n", L.sp_commit_rows(c_, g_, sz(n - cols + 1), sz(h), Zm, sz(rows), sz(cols), blm, out)), ("h_idx = n", L.sp_commit_rows(c_, g_, sz(0), sz(n), Zm, sz(rows), sz(cols), blm, out))])
    _ok(L.sp_commit_rows(c_, g_, sz(0), sz(n), Zm, sz(rows), sz(cols), None, out), "sp_commit_rows, h_idx = n without blinds")      # (h_idx is not looked at then)
    _eq("refusals", bytes(out), want_n, "sp_commit_rows after its refusals")
    ctypes.memset(out, 0xA5, 32 * rows)
    refuse("sp_commit_rows_dev", [
        ("null context", L.sp_commit_rows_dev(None, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, out)), ("null generators", L.sp_commit_rows_dev(c_, None, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, out)),
        ("null table", L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), None, sz(0), sz(rows), sz(cols), blm, out)), ("null out", L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, None)),
        ("no rows", L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), t_, sz(0), sz(0), sz(cols), blm, out)), ("no columns", L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(0), blm, out)),
        ("g_off + cols > n", L.sp_commit_rows_dev(c_, g_, sz(n - cols + 1), sz(h), t_, sz(0), sz(rows), sz(cols), blm, out)), ("h_idx = n", L.sp_commit_rows_dev(c_, g_, sz(0), sz(n), t_, sz(0), sz(rows), sz(cols), blm, out)),
        ("the matrix ends past the table", L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), t_, sz(1), sz(rows), sz(cols), blm, out))])
    _ok(L.sp_commit_rows_dev(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, out), "sp_commit_rows_dev")
    _eq("refusals", bytes(out), want_b, "sp_commit_rows_dev after its refusals")
    ctypes.memset(out, 0xA5, 32 * rows)
    refuse("sp_commit_rows_dev_begin", [
        ("null context", L.sp_commit_rows_dev_begin(None, g_, sz(0), t_, sz(0), sz(rows), sz(cols), jr)), ("null generators", L.sp_commit_rows_dev_begin(c_, None, sz(0), t_, sz(0), sz(rows), sz(cols), jr)),
        ("null table", L.sp_commit_rows_dev_begin(c_, g_, sz(0), None, sz(0), sz(rows), sz(cols), jr)), ("null job", L.sp_commit_rows_dev_begin(c_, g_, sz(0), t_, sz(0), sz(rows), sz(cols), None)),
        ("no rows", L.sp_commit_rows_dev_begin(c_, g_, sz(0), t_, sz(0), sz(0), sz(cols), jr)), ("no columns", L.sp_commit_rows_dev_begin(c_, g_, sz(0), t_, sz(0), sz(rows), sz(0), jr)),
        ("g_off + cols > n", L.sp_commit_rows_dev_begin(c_, g_, sz(n - cols + 1), t_, sz(0), sz(rows), sz(cols), jr)), ("the matrix ends past the table", L.sp_commit_rows_dev_begin(c_, g_, sz(0), t_, sz(1), sz(rows), sz(cols), jr))])
    _ok(L.sp_commit_rows_dev_begin(c_, g_, sz(0), t_, sz(0), sz(rows), sz(cols), jr), "sp_commit_rows_dev_begin")
    _refused(L.sp_job_wait(None, out), "sp_job_wait(NULL)")
    COUNTS["refusals"] += 1
    _eq("refusals", wait(job, rows, "refusals"), want_n, "sp_commit_rows_dev_begin after its refusals")
    job = vp(); jr = ctypes.byref(job)
    refuse("sp_commit_rows_dev_start", [
        ("null context", L.sp_commit_rows_dev_start(None, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, jr)), ("null generators", L.sp_commit_rows_dev_start(c_, None, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, jr)),
        ("null table", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), None, sz(0), sz(rows), sz(cols), blm, jr)), ("null job", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, None)),
        ("8 rows", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), t_, sz(0), sz(8), sz(cols), blm, jr)), ("no columns", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(0), blm, jr)),
        ("g_off + cols > n", L.sp_commit_rows_dev_start(c_, g_, sz(n - cols + 1), sz(h), t_, sz(0), sz(rows), sz(cols), blm, jr)), ("h_idx = n", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(n), t_, sz(0), sz(rows), sz(cols), blm, jr)),
        ("the matrix ends past the table", L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), t_, sz(1), sz(rows), sz(cols), blm, jr))])
    _ok(L.sp_commit_rows_dev_start(c_, g_, sz(0), sz(h), t_, sz(0), sz(rows), sz(cols), blm, jr), "sp_commit_rows_dev_start")
    _eq("refusals", wait(job, rows, "refusals"), want_b, "sp_commit_rows_dev_start after its refusals")
    job = vp(); jr = ctypes.byref(job)
    t2 = capi.Table.alloc(ctx, rows * cols)
    u_ = t2.h
    refuse("sp_commit_rows_upload_start", [
        ("null context", L.sp_commit_rows_upload_start(None, g_, sz(0), sz(h), u_, sz(0), Zm, sz(rows), sz(cols), blm, jr)), ("null generators", L.sp_commit_rows_upload_start(c_, None, sz(0), sz(h), u_, sz(0), Zm, sz(rows), sz(cols), blm, jr)),
        ("null table", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), None, sz(0), Zm, sz(rows), sz(cols), blm, jr)), ("null source", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(0), None, sz(rows), sz(cols), blm, jr)),
        ("null job", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(0), Zm, sz(rows), sz(cols), blm, None)), ("8 rows", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(0), Zm, sz(8), sz(cols), blm, jr)),
        ("no columns", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(0), Zm, sz(rows), sz(0), blm, jr)), ("g_off + cols > n", L.sp_commit_rows_upload_start(c_, g_, sz(n - cols + 1), sz(h), u_, sz(0), Zm, sz(rows), sz(cols), blm, jr)),
        ("h_idx = n", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(n), u_, sz(0), Zm, sz(rows), sz(cols), blm, jr)), ("the matrix ends past the table", L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(1), Zm, sz(rows), sz(cols), blm, jr))])
    assert bytes(t2.download()) == bytes(32 * rows * cols)      # nothing was copied
    _ok(L.sp_commit_rows_upload_start(c_, g_, sz(0), sz(h), u_, sz(0), Zm, sz(rows), sz(cols), blm, jr), "sp_commit_rows_upload_start")
    _eq("refusals", wait(job, rows, "refusals"), want_b, "sp_commit_rows_upload_start after its refusals")
    t2.free()
    job = vp()
    pts = (ctypes.c_uint64 * (16 * 8))()
    refuse("sp_commit_rows_partial", [
        ("null context", L.sp_commit_rows_partial(None, g_, sz(0), t_, sz(0), sz(cols), sz(8), sz(cols), pts)), ("null generators", L.sp_commit_rows_partial(c_, None, sz(0), t_, sz(0), sz(cols), sz(8), sz(cols), pts)),
        ("null table", L.sp_commit_rows_partial(c_, g_, sz(0), None, sz(0), sz(cols), sz(8), sz(cols), pts)), ("null out", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(0), sz(cols), sz(8), sz(cols), None)),
        ("no rows", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(0), sz(cols), sz(0), sz(cols), pts)), ("9 rows", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(0), sz(cols), sz(9), sz(cols), pts)),
        ("no columns", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(0), sz(cols), sz(8), sz(0), pts)), ("z_stride < cols", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(0), sz(cols - 1), sz(8), sz(cols), pts)),
        ("g_off + cols > n", L.sp_commit_rows_partial(c_, g_, sz(n - cols + 1), t_, sz(0), sz(cols), sz(8), sz(cols), pts)),
        ("the last row ends past the table", L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(2), sz(cols + 1), sz(8), sz(cols), pts))])
    assert bytes(pts) == bytes(128 * 8)
    _ok(L.sp_commit_rows_partial(c_, g_, sz(0), t_, sz(1), sz(cols + 1), sz(8), sz(cols), pts), "sp_commit_rows_partial, its last row ending with the table")
    enc = (ctypes.c_uint8 * (32 * 8))()
    _ok(L.sp_host_points_sum_encode(pts, sz(1), sz(8), enc), "sp_host_points_sum_encode")
    from tests.ipa_reference import _msm
    _eq("refusals", bytes(enc), b"".join(_msm(orc, Z[1 + r * (cols + 1):1 + r * (cols + 1) + cols], P[:cols]) for r in range(8)), "sp_commit_rows_partial after its refusals")
    idx = (ctypes.c_uint32 * cols)(*range(cols))
    bad = (ctypes.c_uint32 * cols)(*(list(range(cols - 1)) + [n]))
    refuse("sp_msm_indexed", [
        ("null context", L.sp_msm_indexed(None, g_, idx, sz(cols), Zm, sz(rows), out)), ("null generators", L.sp_msm_indexed(c_, None, idx, sz(cols), Zm, sz(rows), out)),
        ("null indices", L.sp_msm_indexed(c_, g_, None, sz(cols), Zm, sz(rows), out)), ("null scalars", L.sp_msm_indexed(c_, g_, idx, sz(cols), None, sz(rows), out)),
        ("null out", L.sp_msm_indexed(c_, g_, idx, sz(cols), Zm, sz(rows), None)), ("no rows", L.sp_msm_indexed(c_, g_, idx, sz(cols), Zm, sz(0), out)),
        ("no columns", L.sp_msm_indexed(c_, g_, idx, sz(0), Zm, sz(rows), out)), ("an index = n", L.sp_msm_indexed(c_, g_, bad, sz(cols), Zm, sz(rows), out))])
    _ok(L.sp_msm_indexed(c_, g_, idx, sz(cols), Zm, sz(rows), out), "sp_msm_indexed")
    _eq("refusals", bytes(out), want_n, "sp_msm_indexed after its refusals")
    t.free()
