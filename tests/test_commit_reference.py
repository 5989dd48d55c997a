"""CPU checks of tests/commit_reference.py and of the case lists of tests/test_gpu_commit_edges.py: the thresholds the plan restates are still
in the source, the GPU case lists reach every boundary of the row commitments' dispatch on both sides — on a chip of 256 CUs (768 resident
workgroups of the balanced form), of 304 (912) and of 128 (384) — a side no case reaches is shown unreachable over a swept grid, removing any
one class of cases leaves a boundary uncovered, the three boundaries believed unreachable are, issued_tiles equals a per-lane model of
k_msm_q's digit stream whatever the order of the runs, and a row-pool matrix has the commitments of its pool rows."""
import ctypes, itertools, random
import pytest
from tests import commit_reference as CR
from tests import test_gpu_commit_edges as G      # the case lists and the pure-Python case builders: the binding is imported inside its tests
from tests.helpers import Q, gens_bytes, mont_bulk, sz

CHIPS = [(256, 768), (304, 912), (128, 384)]


def test_every_threshold_is_still_in_the_source():
    K = CR.constants()
    assert CR.source_text_missing() == []
    assert K["HMAP_GEN"] == 22528 and K["FLAT_PER_CU"] * 256 == 768
    # a pattern that no longer matches is an error, not a default
    saved = list(CR._PATTERNS)
    try:
        CR._CONST.clear()
        CR._PATTERNS.append(("commit.hip", r"m\.two_pass = m\.P > (\d+) \+ 1;", ("NOT_THERE",)))
        with pytest.raises(AssertionError):
            CR.constants()
    finally:
        CR._PATTERNS[:] = saved
        CR._CONST.clear()
    assert CR.constants() == K


def _csrc(fn):
    import os
    return open(os.path.join(CR._CSRC, fn)).read()


def test_every_rule_and_every_launch_stands_once():
    """one place per decision: every threshold pattern and every restated line of commit.hip and msm_rows.hip occurs exactly once in its file,
    and so do the launches of the latency path's kernels; msm_plan is called from msm_launch and the three job entry points, nowhere else"""
    import re
    for fn, pat, _ in CR._PATTERNS:
        if fn in ("commit.hip", "msm_rows.hip"):
            assert len(re.findall(pat, _csrc(fn))) == 1, (fn, pat)
    for fn in ("commit.hip", "msm_rows.hip"):
        for text in CR.SOURCE_TEXT[fn]:
            assert _csrc(fn).count(text) == 1, (fn, text)
    src = _csrc("commit.hip")
    for launch in ("k_msm_windows_tree_fused,", "(k_msm_windows_tree<true>),", "(k_msm_windows_tree<false>),", "(k_msm_reduce<true, false>),", "k_pt_encode, dim3(1)"):
        assert src.count(launch) == 1, launch
    code = re.sub(r"//.*", "", src)      # (a comment may speak of msm_plan(...))
    callers = []
    for m in re.finditer(r"(?<!static MsmPlan )\bmsm_plan\(", code):
        heads = re.findall(r"^int32_t (\w+)\(", code[:m.start()], re.M)
        callers.append(heads[-1])
    assert callers == ["msm_launch", "sp_commit_rows_dev_begin", "sp_commit_rows_dev_start", "sp_commit_rows_upload_start"], callers


# ------------------------------------------------------------------ reach
# boundary -> predicate over a plan: True | False are its two sides, None: the plan does not come by it
def _in(form):
    return lambda p: p["form"] in form


TREE = ("tree1", "tree_fused", "tree_unfused")
BOUNDARIES = {
    "lookup | throughput line at <= 8 rows": lambda p: p["windowed"] if p["rows"] == 8 else None,
    "lookup | throughput line above 8 rows": lambda p: p["windowed"] if p["rows"] == 9 else None,
    "rows 8 | 9 in a lookup shape": lambda p: p["form"] in TREE if p["windowed"] and p["rows"] in (8, 9) else None,
    "one | more workgroups per row of the tree": lambda p: p["nblk"] == 1 if p["form"] in TREE and p["P"] in (256, 288) else None,
    "256 | 257 workgroups per row of the tree": lambda p: p["tree_reduce_strided"] if p["form"] in TREE and p["nblk"] in (256, 257) else None,
    "fused | unfused tree": lambda p: p["form"] == "tree_fused" if p["form"] in TREE and p["nblk"] > 1 else None,
    "host | device encode of one workgroup per row": lambda p: p["encode"] == "host" if p["form"] == "tree1" else None,
    "one | two reduction passes (lookup form)": lambda p: p["two_pass"] if p["form"] == "windows" and p["P"] in (2040, 2091) else None,
    "one | two reduction passes (strip form, few rows)": lambda p: p["two_pass"] if p["form"] == "strip" and p["rows"] <= 8 else None,
    "a last chunk shorter than 256": lambda p: p["last_chunk"] < 256 if p["two_pass"] else None,
    "encode in the reduction | one lane per row (lookup)": lambda p: p["encode"] == "batch" if p["windowed"] and p["rows"] in (63, 64) else None,
    "encode in the reduction | one lane per row (throughput)": lambda p: p["encode"] == "batch" if not p["windowed"] and p["rows"] in (63, 64) else None,
    "result page | staging copy (lookup)": lambda p: p["small_out"] if p["windowed"] and p["rows"] in (1024, 1025) and p["role"] == "sync" else None,
    "result page | staging copy (throughput)": lambda p: p["small_out"] if not p["windowed"] and p["rows"] in (1024, 1025) and p["role"] == "sync" else None,
    "lean encode of the co-resident background launch": lambda p: p["encode"] == "batch_lean" if p["form"] == "queue" and p["rows"] >= 64 else None,
    "device encode of a few-row throughput shape": lambda p: p["encode"] == "batch" if not p["windowed"] and p["rows"] <= 8 else None,
    "strip: xcd order": lambda p: p["xcd"] if p["form"] in ("strip", "strip_bg") and p["rows"] >= 255 else None,
    "strip: xcd order with idle tiles": lambda p: p["xcd_idle"] if p["form"] in ("strip", "strip_bg") and p["xcd"] else None,
    "strip: one | two columns per strip": lambda p: p["strip"] == 2 and p["last_strip"] == 1 if p["form"] == "strip" and p["rows"] >= 255 else None,
    "strip: persistent background launch | plain": lambda p: p["form"] == "strip_bg" if p["form"] in ("strip", "strip_bg") and p["role"] == "begin" else None,
    "strip | flat at 256 rows under msm.form = 3": lambda p: p["form"] == "flat" if p["rows"] in (255, 256) and not p["windowed"] and p["opt_form"] == 3 and p["role"] == "sync" else None,
    "flat: four | five row-blocks": lambda p: p["form"] == "flat" if p["rows"] in (1024, 1280) and p["form"] in ("strip", "flat") and p["role"] == "sync" else None,
    "flat: runs clamped by units / 4 | by the resident workgroups": lambda p: p["flat_by_units"] if p["form"] == "flat" else None,
    "flat: runs that do not divide the units": lambda p: True if p["form"] == "flat" and p["flat_uneven"] else None,
    "flat: one | several row-blocks per launch": lambda p: p["flat_rb"] == 1 if p["form"] == "flat" else None,
    "flat: not next to a background commit": lambda p: p["form"] == "flat" if p["rows"] == 256 and p["role"] == "start" and p["form"] in ("strip", "flat") else None,
    "upload: chunked | copy-then-commit": lambda p: p["chunked"] if p["role"] == "upload" else None,
    "upload: one | several chunks": lambda p: p["nlaunch"] == 1 if p["role"] == "upload" and p["chunked"] else None,
    "queue: 255 | 256 rows": lambda p: p["form"] == "queue" if p["rows"] in (255, 256) and p["opt_form"] == 0 and not p["windowed"] and p["role"] == "sync" else None,
    "queue: 1024 | 1025 row groups": lambda p: p["form"] == "queue" if p["rows"] in (65536, 65600) else None,
    "queue: a last group that is no whole wavefront": lambda p: p["rows"] % 64 != 0 if p["form"] == "queue" else None,
    "queue: small-launch recut": lambda p: p["recut"] if p["form"] == "queue" else None,
    "queue: the floor of four units": lambda p: p["len_floored"] if p["form"] == "queue" else None,
    "queue: a clipped last run": lambda p: p["last_run_clipped"] if p["form"] == "queue" else None,
    "queue: fewer workgroups than CUs": lambda p: p["wgs_clipped"] if p["form"] == "queue" else None,
    "queue: alone | co-resident": lambda p: p["coresident"] if p["form"] == "queue" else None,
    "queue: 4 | 12 wavefronts": lambda p: p["waves"] == 4 if p["form"] == "queue" and p["waves"] in (4, 12) else None,
    "queue: through the upload in one chunk (the slot counts must reach the reduction)": lambda p: p["counts_in_reduce"] and p["role"] == "upload" if p["form"] == "queue" else None,
    "queue: runs that begin inside a scalar": lambda p: True if p["form"] == "queue" and p["len"] % 51 != 0 else None,
    "lds: 511 | 512 rows": lambda p: p["form"] == "lds" if p["rows"] in (511, 512) and not p["windowed"] and p["opt_form"] == 1 else None,
    "lds: 768 | 769 rows (4 | 3 loader wavefronts)": lambda p: p["loaders"] == 4 if p["form"] == "lds" and p["rows"] in (768, 769) else None,
    "lds: 960 | 961 rows (1 | 0 loader wavefronts)": lambda p: p["loaders"] == 1 if p["form"] == "lds" and p["rows"] in (960, 961) else None,
    "lds: one | two row-blocks": lambda p: p["nrb"] == 1 if p["form"] == "lds" and p["launch_rows"] in (1024, 1025) else None,
    "lds: two | three row-blocks": lambda p: p["nrb"] == 2 if p["form"] == "lds" and p["launch_rows"] in (2048, 2049) else None,
    "lds: runs clamped by units / 4 | by the workgroup slots": lambda p: p["lds_by_units"] if p["form"] == "lds" else None,
    "lds: the background grid limit": lambda p: p["grid_limited"] if p["form"] == "lds" and p["role"] == "begin" else None,
    "lds: next to a background commit": lambda p: p["role"] == "start" and p["P"] != 0 if p["form"] == "lds" and p["role"] in ("start", "sync") else None,
}


ONE_SIDED = {"queue: runs that begin inside a scalar", "flat: runs that do not divide the units"}      # a property the cases must have, not a branch


def _plans(cases, chip):
    return [p for c in cases for p in G.plans_of(c, *chip)]


def uncovered(cases, chip):
    """the (boundary, side) pairs no plan of the cases comes by"""
    seen = set()
    for p in _plans(cases, chip):
        for name, pred in BOUNDARIES.items():
            v = pred(p)
            if v is not None:
                seen.add((name, bool(v)))
    return sorted((n, s) for n in BOUNDARIES for s in (True, False) if (n, s) not in seen and not (n in ONE_SIDED and not s))


def _sweep(chip):
    """a grid over the arguments of plan(): shapes on and around every row threshold, 1..130 columns, the three window counts of the GPU
    sets, every form option and role"""
    rows = [1, 8, 9, 63, 64, 255, 256, 257, 320, 511, 512, 768, 769, 960, 961, 1024, 1025, 1280, 2048, 2049, 4096, 65536, 65600]
    opts = [{}, {"form": 3}, {"form": 1}, {"q_waves": 4}, {"q_units": 4}, {"q_units": 4096}, {"device_encode": 1}, {"upload_chunks": 1}, {"bg_eighths": 1, "form": 1}]
    for r, ncol, nwin, o, role, blind in itertools.product(rows, list(range(1, 131)) + [513, 1285, 1286, 2049], (17, 32, 51), opts, CR.ROLES, (0, 1)):
        if role != "sync" and (r <= 8 or (o.get("device_encode") and role != "sync")):
            continue
        if ncol - blind < 1 or (blind and role == "begin"):
            continue
        yield CR.plan(r, ncol - blind, blind, nwin, o, chip[0], chip[1], 26 if o.get("form") == 1 else None, role)


@pytest.mark.parametrize("chip", CHIPS, ids=["%dcu" % c[0] for c in CHIPS])
def test_gpu_cases_reach_both_sides_of_every_boundary(chip):
    """on the chip the shapes were derived for, every side is reached; on the other two, a side the cases miss must be out of reach of ANY shape
    of the swept grid (the queue form's floor of four units cannot be met on 128 CUs: a commit with so few units per resident wavefront is
    lookup-sized)"""
    miss = uncovered(G.ALL_CASES, chip)
    if chip == CHIPS[0]:
        assert miss == [], miss
    if miss:
        reachable = set()
        for p in _sweep(chip):
            for name, side in miss:
                v = BOUNDARIES[name](p)
                if v is not None and bool(v) == side:
                    reachable.add((name, side))
        assert not reachable, ("sides the sweep reaches and no case does", sorted(reachable))
        assert len(miss) <= 2, miss      # exemptions stay the exception


def test_every_case_takes_the_form_its_section_is_about():
    for chip in CHIPS:
        for c in G.ALL_CASES:
            forms = [p["form"] for p in G.plans_of(c, *chip)]
            if c.sec == "tree":
                assert all(f in TREE + ("windows",) for f in forms), c.name
            if c.sec == "strip":
                assert all(f in ("strip", "strip_bg") for f in forms), c.name
            if c.sec == "digits":
                assert all(f in ("flat", "queue", "strip", "lds") for f in forms) and all(not p["windowed"] for p in G.plans_of(c, *chip)), c.name
            if c.sec == "reduce":
                assert forms == ["windows"], c.name
    # the digits go through every form that rebuilds a carry in the middle of a scalar, at every geometry
    for w, n in G.DIGIT_GEOMS:
        got = {p["form"] for c in G.DIGIT_CASES if c.set == "g_%d_%d" % (w, n) for p in G.plans_of(c, *CHIPS[0])}
        assert got == {"flat", "queue", "strip"}, (w, n, got)
    assert {c.set for c in G.DIGIT_CASES if G.plans_of(c, *CHIPS[0])[0]["form"] == "lds"} == {"l6", "l10"}
    # every product columns x windows below 300 the three geometries give
    for s, nwin in (("w5", 51), ("n32", 32), ("dflt", G.DEFAULT_WINDOWS)):
        assert {G.plans_of(c, *CHIPS[0])[0]["P"] for c in G.SMALL_P_CASES if c.set == s} == {k * nwin for k in range(1, 300) if k * nwin < 300}, s
    # names are unique (they are the test ids), and every set holds the generators its cases name
    assert len({c.name for c in G.ALL_CASES}) == len(G.ALL_CASES)
    assert all(c.cols + 1 <= G.SETS[c.set][0] for c in G.ALL_CASES)


SECTIONS = ["TREE_CASES", "LINE_CASES", "REDUCE_CASES", "ENCODE_CASES", "STRIP_CASES", "FLAT_CASES", "QUEUE_CASES", "LDS_CASES"]


@pytest.mark.parametrize("dropped", SECTIONS)
def test_removing_a_class_of_cases_uncovers_a_boundary(dropped):
    rest = [c for c in G.ALL_CASES if c not in getattr(G, dropped)]
    assert uncovered(rest, CHIPS[0]) != [], dropped


def test_removing_any_single_queue_or_lds_row_count_uncovers_a_boundary():
    """the row counts of the issue's lists, one at a time"""
    for rows in (255, 256, 65536, 65600, 511, 512, 769, 960, 961, 1025, 2049, 63, 64):
        rest = [c for c in G.ALL_CASES if c.rows != rows]
        assert uncovered(rest, CHIPS[0]) != [], rows


# ------------------------------------------------------------------ the three boundaries believed unreachable
@pytest.mark.parametrize("chip", CHIPS, ids=["%dcu" % c[0] for c in CHIPS])
def test_boundaries_believed_unreachable_are(chip):
    K = CR.constants()
    # 1. `counts` inside k_pt_reduce_pass: the queue form never has more than 2048 partial sums per row (S <= share + 64, share <= workers / 4)
    worst = 0
    for rows in list(range(256, 4097, 64)) + [257, 65536]:
        for waves in (4, 8, 12):
            for ncol in (1, 41, 4096):
                q = CR.q_cut(rows, ncol, 51, waves, 32, chip[0])
                worst = max(worst, q["S"])
    assert worst <= _cdiv(chip[0] * 12, 4) + K["Q_STEAL"] < K["TWO_PASS"]
    assert not any(p["counts_in_pass"] for p in _sweep(chip))
    # 2. the k = 4..npieces tail of the hooked DMA in msm_lds_run: a workgroup without loader wavefronts has 16 wavefronts, and a sub-table
    # of at most 10 bits has 48 pieces: three per wavefront
    for bits in range(6, 11):
        for rows in range(K["LDS_MIN_ROWS"], 4200):
            assert CR.lds_hook_tail(bits, rows) == 0, (bits, rows)
    # 3. strip > cols: total / 524288 > cols needs more than 2^19 rows; the clamp then leaves nstrips = 1 and every column in the one strip,
    # which the kernel's own `if (j1 > cols) j1 = cols` gives as well: no launch changes
    assert not any(p.get("strip_over_cols") for p in _sweep(chip))
    for rows, cols in ((1 << 19, 7), ((1 << 19) + 1, 1), ((1 << 19) + (1 << 16), 9)):
        p = CR.plan(rows, cols, 0, 51, {"form": 3}, chip[0], chip[1])
        assert p["strip_over_cols"] == (rows * cols // K["TARGET_THREADS"] > cols) and p["nstrips"] == (1 if p["strip_over_cols"] else _cdiv(cols, p["strip"]))
    assert CR.plan((1 << 19) + (1 << 16), 9, 0, 51, {"form": 3}, chip[0], chip[1])["strip_over_cols"]


def _cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the plan against hand-worked shapes
def test_plan_on_shapes_worked_by_hand():
    P = lambda r, c, b=0, nwin=51, role="sync", lds=None, **o: CR.plan(r, c, b, nwin, o, 256, 768, lds, role)
    assert P(1, 5)["form"] == "tree1" and P(1, 6)["form"] == "tree_fused" and P(1, 6, device_encode=1)["form"] == "tree_unfused"
    assert P(1, 1285)["nblk"] == 256 and P(1, 1286)["nblk"] == 257 and P(1, 1286)["last_block"] == 65586 - 256 * 256
    assert P(8, 1285)["windowed"] and not P(8, 1286)["windowed"] and P(9, 1142)["windowed"] and not P(9, 1143)["windowed"]
    p = P(8, 2049)
    assert (p["form"], p["P"], p["two_pass"], p["nchunks"], p["last_chunk"], p["encode"]) == ("strip", 2049, True, 3, 1, "host")
    p = P(9, 41)
    assert (p["form"], p["P"], p["two_pass"], p["nchunks"], p["last_chunk"]) == ("windows", 2091, True, 3, 43)
    p = P(2048, 513, form=3)
    assert (p["form"], p["strip"], p["nstrips"], p["last_strip"], p["xcd"], p["nblocks"]) == ("strip", 2, 257, 1, True, 33 * 8 * 8)
    p = P(1280, 11, form=3)
    assert (p["form"], p["nstrips"], p["xcd_idle"], p["nblocks"]) == ("strip", 11, True, 2 * 8 * 5)
    p = P(300, 41, form=3)
    assert (p["xcd"], p["nblocks"]) == (False, _cdiv(300 * 41, 256))
    assert P(256, 41, form=3)["P"] == 2091 // 4 and P(256, 61, form=3)["P"] == 768 and P(1024, 12, 1, form=3)["P"] == 13 * 51 // 4 and P(1024, 40, form=3)["P"] == 192
    p = P(256, 41, 1)
    assert (p["form"], p["share"], p["len"], p["nb"], p["S"], p["wgs"]) == ("queue", 768, 4, 536, 832, 179)
    p = P(65536, 1, 1)
    assert (p["form"], p["ngroups"], p["share"], p["len"], p["nb"], p["S"], p["wgs"]) == ("queue", 1024, 3, 32, 4, 67, 256)
    assert P(65600, 1, 1)["form"] == "strip"
    assert CR.lds_shape(768) == (1, 768, 1024, 4) and CR.lds_shape(769) == (1, 769, 1024, 3) and CR.lds_shape(960) == (1, 960, 1024, 1)
    assert CR.lds_shape(961) == (1, 961, 1024, 0) and CR.lds_shape(1025) == (2, 513, 832, 4) and CR.lds_shape(2049) == (3, 683, 960, 4)
    p = P(40000, 1, 0, role="begin", lds=26, form=1, bg_eighths=1)
    assert (p["form"], p["nrb"], p["P"], p["n_wg"], p["grid"], p["grid_limited"]) == ("lds", 40, 1, 40, 32, True)
    assert CR.indexed_staging(1, 625) and not CR.indexed_staging(1, 626) and CR.indexed_staging(9, 77) and not CR.indexed_staging(9, 78)
    for rows, cols in G.INDEXED_CASES:
        assert CR.indexed_staging(rows, cols) == (cols in (625, 331, 86, 77)), (rows, cols)


# ------------------------------------------------------------------ the tiles of the queue form
def lane_model_tiles(Z, rows, cols, blind, geom, ln, order):
    """k_msm_q's loop written out per lane: a 256-bit register shifted window by window, the carry rebuilt from window 0 for a run that starts
    inside a scalar, the ballot over the 64 lanes of the group in front of every tile"""
    ncol = cols + (1 if blind is not None else 0)
    U = ncol * geom.nwin
    n = 0
    for grp, bk in order:
        u, u1 = bk * ln, min((bk + 1) * ln, U)
        j0, j1 = u // geom.nwin, (u1 - 1) // geom.nwin
        w_first, w_last = u % geom.nwin, (u1 - 1) % geom.nwin + 1
        for j in range(j0, j1 + 1):
            lanes = []
            for lane in range(64):
                r = grp * 64 + lane
                lanes.append([0 if r >= rows else (Z[r * cols + j] if j < cols else blind[r]), 0])      # [remaining scalar, carry]
            w = 0

            def step(st, w):
                c = geom.width(w)
                d = (st[0] & ((1 << c) - 1)) + st[1]
                st[1] = 1 if d >= (1 << (c - 1)) else 0
                st[0] >>= c
            if j == j0:
                while w < w_first:
                    for st in lanes:
                        step(st, w)
                    w += 1
            w_end = w_last if j == j1 else geom.nwin
            while w < w_end:
                if all(st[0] == 0 and st[1] == 0 for st in lanes):
                    break
                for st in lanes:
                    step(st, w)
                n += 1
                w += 1
    return n


@pytest.mark.parametrize("wbits,windows", [(5, 0), (0, 32), (0, 17), (13, 0)])
def test_issued_tiles_equals_the_per_lane_model_in_any_run_order(wbits, windows):
    ge = CR.Geom(wbits=wbits, windows=windows)
    rng = random.Random(wbits * 100 + windows)
    pool = CR.digit_pool(ge) + CR.edge_pool()
    for rows, cols, with_blind, ln, kind in [(130, 3, True, 4, "pool"), (64, 2, False, 5, "short"), (200, 2, True, 32, "zero"), (70, 3, False, 4096, "pool"), (65, 1, True, 7, "short")]:
        if kind == "pool":
            Z = [pool[rng.randrange(len(pool))] for _ in range(rows * cols)]
        else:
            Z = [rng.getrandbits(rng.choice((1, 7, 33))) for _ in range(rows * cols)]
        if kind == "zero":      # a whole zero group, and a group with one live row
            Z = [rng.randrange(Q) if r < 64 or r == 150 else 0 for r in range(rows) for _ in range(cols)]
        blind = [pool[rng.randrange(len(pool))] if kind != "zero" or r < 64 else 0 for r in range(rows)] if with_blind else None
        U = (cols + (1 if with_blind else 0)) * ge.nwin
        items = [(g, bk) for g in range(_cdiv(rows, 64)) for bk in range(_cdiv(U, ln))]
        want = lane_model_tiles(Z, rows, cols, blind, ge, ln, items)
        assert CR.issued_tiles(Z, rows, cols, blind, ge, ln) == want, (rows, cols, ln, kind)
        for _ in range(3):      # whichever wavefront takes a run, in whatever order: the same count
            rng.shuffle(items)
            assert CR.issued_tiles(Z, rows, cols, blind, ge, ln, order=list(items)) == want
            assert lane_model_tiles(Z, rows, cols, blind, ge, ln, items) == want
        if kind == "pool":
            assert want < _cdiv(rows, 64) * U or any(CR.live_windows(s, ge) == ge.nwin for s in Z)
    # a short scalar needs only its low windows; a carry out of the top bit of a field needs one window more
    assert CR.live_windows(0, ge) == 0 and CR.live_windows(1, ge) == 1 and CR.live_windows(ge.half(0), ge) == 2 and CR.live_windows(ge.half(0) - 1, ge) == 1
    assert CR.live_windows(Q - 1, ge) == ge.nwin


# ------------------------------------------------------------------ row pools
def test_row_pool_matrix_and_its_expected_commitments(orc):
    rng = random.Random(9)
    cols, n = 3, 65
    comp = gens_bytes(orc, cols, b"gens_commit_reference")
    pool = [CR.edge_vector(cols, rng) for _ in range(n)]
    blinds = CR.edge_vector(n, rng)
    assert len({tuple(r) for r in pool}) > 50
    Z, idx = CR.row_pool_matrix(pool, 700)
    assert idx == [(r * 7) % n for r in range(700)] and Z == [x for i in idx for x in pool[i]]
    groups = [tuple(idx[g:g + 64]) for g in range(0, 640, 64)]
    assert all(len(set(g)) == 64 for g in groups) and len(set(groups)) == len(groups)      # distinct rows in a group, no two groups alike
    for bad in (pool[:64], pool[:63], pool + pool[:5]):      # even, not above a wavefront, a multiple of the stride
        with pytest.raises(AssertionError):
            CR.row_pool_matrix(bad, 100)
    got = CR.expected(orc, comp[:32 * cols], comp[32 * cols:], pool, idx[:150], blinds)
    want = (ctypes.c_uint8 * (32 * 150))()
    assert orc.orc_commit_rows(comp[:32 * cols], sz(cols), comp[32 * cols:], mont_bulk(Z[:150 * cols]), sz(150), sz(cols), mont_bulk([blinds[i] for i in idx[:150]]), want) == 0
    assert got == bytes(want)
    assert CR.expected(orc, comp[:32 * cols], comp[32 * cols:], [[0] * cols], [0, 0]) == CR.NEUTRAL * 2


def test_case_matrices_hold_every_value_of_their_pool():
    for c in G.DIGIT_CASES + [G.K("queue", "w5", 256, 41, 1)]:
        Z, bl = G.flat_matrix(c)
        assert set(G.value_pool(c.set)) <= set(Z), c.name
    z = G.K("queue", "w5", 321, 41, 1, "sync", "zero_groups")
    Z, bl = G.flat_matrix(z)
    live = [any(Z[r * 41:(r + 1) * 41]) or bl[r] != 0 for r in range(321)]
    assert all(live[:64]) and not any(live[64:128]) and sum(live[128:192]) == 1 and not any(live[192:256]) and all(live[256:320])
    s = G.K("queue", "w5", 321, 41, 1, "sync", "short")
    assert max(G.flat_matrix(s)[0]) < 1 << 33
