"""The dispatch of the fixed-base row commitments (sp_commit_rows*, sp_msm_indexed, sp_commit_rows_partial: spartan_amd/csrc/commit.hip,
msm_rows.hip, msm_queue.hip, msm_lds.hip) restated in Python integers for tests/test_commit_reference.py (CPU) and
tests/test_gpu_commit_edges.py. No device; ctypes only to call the oracle handle a function is given.

  constants          every literal threshold of the dispatch, read from the source text (a line that was re-expressed raises)
  plan               msm_plan, the branches of msm_launch, msm_enqueue_reduce, msm_q_cut, msm_q_enqueue's workgroup clip, msm_lds_shape,
                     msm_lds_runs and the strip / xcd arithmetic of msm_rows_enqueue: which kernels a call runs, on what grid
  issued_tiles       the exact number of tiles k_msm_q issues for a matrix (what sp_prof_read_spans reports, divided by 64)
  row_pool_matrix    a tall matrix whose rows come from a small pool of distinct rows; expected: its commitments from one oracle call over
                     the pool (a commitment depends on its own row only)
Window geometry, digits and the edge-value pools are those of tests/ipa_reference.py (Geom, digit_pool, edge_pool, edge_vector)."""
import ctypes, math, os, re
from tests.helpers import Q, ROOT, mont_bulk, sz
from tests.ipa_reference import Geom, digit_pool, edge_pool, edge_vector      # re-exported: the GPU module takes them from here

NEUTRAL = bytes(32)      # RFC 9496 encoding of the neutral element
_CSRC = os.path.join(ROOT, "spartan_amd", "csrc")
# (file, regular expression with one group per constant, names)
_PATTERNS = [
    ("internal.hpp", r"constexpr size_t HMAP_IN = (\d+), HMAP_SIZE = (\d+), EQ_SLOTS = (\d+), EQ_SLOT_BYTES = (\d+), HMAP_GEN = HMAP_IN - EQ_SLOTS \* EQ_SLOT_BYTES;",
     ("HMAP_IN", "HMAP_SIZE", "EQ_SLOTS", "EQ_SLOT_BYTES")),
    ("internal.hpp", r"constexpr size_t SP_HOST_ENCODE_ROWS = (\d+);", ("HOST_ENCODE_ROWS",)),
    ("internal.hpp", r"constexpr unsigned MSMQ_MAX_GROUPS = (\d+),", ("Q_MAX_GROUPS",)),
    ("ctx.hip", r"c->bg_blocks = c->n_cus \* \(int\)c->opt\.v\[OPT_BG_EIGHTHS\] / (\d+);", ("BG_DENOM",)),
    ("commit.hip", r"m\.windowed = rows \* ncol \* NWIN <= \(\(size_t\)1 << (\d+)\);", ("WINDOWED_LOG2",)),
    ("commit.hip", r"const size_t target_threads = (\d+);", ("TARGET_THREADS",)),
    ("commit.hip", r"if \(rows % (\d+) == 0 && launch_rows % (\d+) == 0 && launch_rows / (\d+) <= (\d+) && !bg_subblocks && !shares_chip\) \{\n\s*const size_t rb = launch_rows / (\d+), units = ncol \* NWIN;",
     ("FLAT_ROWS", "FLAT_ROWS2", "FLAT_ROWS3", "FLAT_MAX_BLOCKS", "FLAT_ROWS4")),
    ("commit.hip", r"if \(nb > units / (\d+)\) nb = units / (\d+);       // at least four additions per thread", ("FLAT_MIN_UNITS", "FLAT_MIN_UNITS2")),
    ("commit.hip", r"\(opt\.v\[OPT_MSM_FORM\] == 0 && g->prefer_lds\)\) && launch_rows >= (\d+)\) \{", ("LDS_MIN_ROWS",)),
    ("commit.hip", r"size_t slots = bg_subblocks \? bg_subblocks / (\d+) : \(shares_chip \? (\d+) \* cus : cus\);", ("LDS_BG_DIV", "LDS_SHARE_MULT")),
    ("commit.hip", r"launch_rows >= (\d+) && launch_rows == rows && \(rows \+ (\d+)\) / (\d+) <= MSMQ_MAX_GROUPS\) \{", ("Q_MIN_ROWS", "Q_GROUP_ROUND", "Q_GROUP")),
    ("commit.hip", r"m\.chunk = (\d+); m\.nchunks = \(m\.P \+ m\.chunk - 1\) / m\.chunk;\n  m\.two_pass = m\.P > (\d+);", ("CHUNK", "TWO_PASS")),
    ("commit.hip", r"const bool batch_encode = encode && rows >= (\d+) && sums_extra != nullptr;", ("BATCH_ROWS",)),
    ("commit.hip", r"size_t nblk = \(m\.P \+ (\d+)\) / (\d+);", ("TREE_ROUND", "TREE_BLOCK")),
    ("commit.hip", r"pt10_tree_quad\(sm, xch, nblk < (\d+) \? nblk : (\d+)\);", ("TREE_REDUCE", "TREE_REDUCE2")),
    ("commit.hip", r"MsmPlan m = msm_plan\(c, g, rows, cols, false, c->bg_blocks > 0 \? \(size_t\)c->bg_blocks \* (\d+) : 0\);", ("BG_SUBBLOCKS",)),
    ("commit.hip", r"if \(counts && !IN10 && counts\[row / (\d+)\] < nstrips\) nlive = counts\[row / (\d+)\];", ("COUNT_GROUP", "COUNT_GROUP2")),
    ("msm_queue.hip", r"if \(len < (\d+)\) len = (\d+);", ("Q_MIN_LEN", "Q_MIN_LEN2")),
    ("msm_queue.hip", r"r\.S = \(unsigned\)\(share \+ (\d+)\);", ("Q_STEAL",)),
    ("msm_queue.hip", r"const size_t workers = wgs \* waves, ngroups = \(rows \+ (\d+)\) / (\d+);", ("Q_CUT_ROUND", "Q_CUT_GROUP")),
    ("msm_lds.hip", r"size_t b = \(rows \+ (\d+)\) / (\d+);\n  size_t per = \(rows \+ b - 1\) / b;\n  size_t t = \(per \+ (\d+)\) / (\d+) \* (\d+);\n  for \(int k = 0; k < (\d+) && t \+ (\d+) <= (\d+); k\+\+\) t \+= (\d+);",
     ("LDS_WG_ROUND", "LDS_WG", "LDS_WAVE_ROUND", "LDS_WAVE", "LDS_WAVE2", "LDS_LOADERS", "LDS_WAVE3", "LDS_WG2", "LDS_WAVE4")),
    ("msm_lds.hip", r"if \(nb > units / (\d+)\) nb = units / (\d+);  // at least four tiles per run", ("LDS_MIN_UNITS", "LDS_MIN_UNITS2")),
    ("msm_lds.hip", r"if \(more\) for \(unsigned k = (\d+); k < npieces; k\+\+\) dma_piece\(src, buf \^ 1u, k\);", ("LDS_HOOKS",)),
    ("msm_rows.hip", r"int xcd_map = rows % (\d+) == 0;\n  size_t nblocks = xcd_map \? \(\(nstrips \+ (\d+)\) / (\d+)\) \* (\d+) \* \(rows / (\d+)\) : \(rows \* nstrips \+ (\d+)\) / (\d+);",
     ("XCD_ROWS", "XCD_ROUND", "XCD", "XCD2", "XCD_ROWS2", "STRIP_ROUND", "STRIP_BLOCK")),
    ("msm_rows.hip", r"if \(e != hipSuccess \|\| per_cu < 1\) per_cu = (\d+);", ("FLAT_PER_CU",)),
]
# text the plan restates without a number of its own in it
SOURCE_TEXT = {
    "commit.hip": [
        "if (m.strip < 1) m.strip = 1;",
        "if (m.strip > cols) m.strip = cols;",
        "m.strip = total / target_threads;",
        "size_t nb = msm_flat_slots() / rb;",
        "if (nb >= 1) { m.flat = 2; m.P = nb; }",
        "if (g->table_lds && (opt.v[OPT_MSM_FORM] == 1 || (opt.v[OPT_MSM_FORM] == 0 && g->prefer_lds))",
        "} else if ((opt.v[OPT_MSM_FORM] == 0 || opt.v[OPT_MSM_FORM] == 2) && launch_rows >= ",
        "m.qrole = bg_subblocks || shares_chip ? MSMQ_CORESIDENT : MSMQ_ALONE;",
        "const bool encode_in_reduce = encode && !batch_encode;",
        "if (m.queue && m.qrole == MSMQ_CORESIDENT && st != c->stream)",
        "if (nblk > 1 && !c->device_encode && c->done_counter) {",
        "if (rows <= SP_HOST_ENCODE_ROWS) {  // latency path",
        "bool small_out = 32 * rows <= HMAP_SIZE - HMAP_IN;",
        "hipLaunchKernelGGL(k_pt_reduce_pass, dim3((unsigned)rows, (unsigned)m.nchunks), dim3(256), 0, st, (const Pt*)partial, m.P, m.chunk, partial2, qcounts);",
        "MsmPlan m = msm_plan(c, g, rows, cols, blinds != nullptr, 0, chunked_on && rows % (256 * nch) == 0 ? rows / nch : 0, c->bg_inflight > 0);",
        "if (!chunked_on || m.windowed || rows % (256 * nch) != 0) {",
        "true, j->scratch + lay.sums_off, nch == 1 ? qcounts : nullptr);",
        "if (sb + ib <= HMAP_GEN) {",
        "size_t sb = 32 * rows * cols, ib = (4 * cols + 31) & ~(size_t)31;",
        "msm_lds_enqueue(c, st, g, dZ, z_stride, rows, cols, g_off, didx, dblinds, h_idx, partial, m.P, st != c->stream && c->bg_blocks > 0 ? (unsigned)c->bg_blocks : 0u);",
    ],
    "msm_queue.hip": [
        "unsigned wv = (unsigned)c->opt.v[role != MSMQ_ALONE ? OPT_MSM_Q_BG_WAVES : OPT_MSM_Q_WAVES], d = MSMQ_D;",
        "*wgs = (size_t)c->n_cus;",
        "const size_t share = (workers + ngroups - 1) / ngroups;",
        "if (len * share > units) len = (units + share - 1) / share;",
        "r.nb = (unsigned)((units + len - 1) / len);",
        "if (r.S > workers) r.S = (unsigned)workers;",
        "const size_t need = ((size_t)A.nb * A.ngroups + waves - 1) / waves;",
        "if (wgs > need) wgs = need;",
        "if (__all((s0 | s1 | s2 | s3) == 0 && carry == 0)) break;",
        "if (u1 > U) u1 = U;",
    ],
    "msm_lds.hip": [
        "size_t nb = wg_slots / nrb;",
        "if (nb < 1) nb = 1;",
        "if (grid_limit && grid > grid_limit) grid = grid_limit;",
        "const unsigned npieces = ((sub_bytes >> 10) + (T >> 6) - 1) / (T >> 6);",
        "if (nload == 0 && p < kb) piece(src, buf, p);",
        "const unsigned nload = nwaves > nlive ? nwaves - nlive : 0;",
    ],
    "msm_rows.hip": [
        "if (st != c->stream && !didx && !dblinds && c->bg_blocks > 0) {",
        "if (j1 > cols) j1 = cols;",
        "return slots[dev] = (size_t)per_cu * (size_t)prop.multiProcessorCount;",
    ],
}
_CONST = {}


def constants():
    """the literal thresholds of the dispatch, read from the source: a changed number changes every plan below (and
    tests/test_commit_reference.py then finds a boundary uncovered); a line the reader cannot find is an error, never a default"""
    if not _CONST:
        K = {}
        for fn, pat, names in _PATTERNS:
            src = open(os.path.join(_CSRC, fn)).read()
            m = re.search(pat, src)
            if not m:
                raise AssertionError("%s no longer contains /%s/: restate tests/commit_reference.py" % (fn, pat))
            K.update({k: int(v) for k, v in zip(names, m.groups())})
        K["HMAP_GEN"] = K["HMAP_IN"] - K["EQ_SLOTS"] * K["EQ_SLOT_BYTES"]
        # one number written several times in one expression: the restatement below uses one name for it
        assert K["FLAT_ROWS"] == K["FLAT_ROWS2"] == K["FLAT_ROWS3"] == K["FLAT_ROWS4"] == K["XCD_ROWS"] == K["XCD_ROWS2"] == K["STRIP_BLOCK"] == K["TREE_BLOCK"]
        assert K["FLAT_MIN_UNITS"] == K["FLAT_MIN_UNITS2"] and K["LDS_MIN_UNITS"] == K["LDS_MIN_UNITS2"] and K["Q_MIN_LEN"] == K["Q_MIN_LEN2"]
        assert K["TREE_ROUND"] == K["TREE_BLOCK"] - 1 == K["STRIP_ROUND"] and K["TREE_REDUCE"] == K["TREE_REDUCE2"] == K["TREE_BLOCK"]
        assert K["Q_GROUP"] == K["Q_CUT_GROUP"] == K["COUNT_GROUP"] == K["COUNT_GROUP2"] == 64 and K["Q_GROUP_ROUND"] == K["Q_CUT_ROUND"] == 63
        assert K["LDS_WG"] == K["LDS_WG2"] == K["LDS_WG_ROUND"] + 1 and K["LDS_WAVE"] == K["LDS_WAVE2"] == K["LDS_WAVE3"] == K["LDS_WAVE4"] == K["LDS_WAVE_ROUND"] + 1 == 64
        assert K["XCD"] == K["XCD2"] == K["XCD_ROUND"] + 1
        _CONST.update(K)
    return _CONST


def source_text_missing():
    out = []
    for fn, texts in SOURCE_TEXT.items():
        src = open(os.path.join(_CSRC, fn)).read()
        out += [(fn, t) for t in texts if t not in src]
    return out


# ------------------------------------------------------------------ the plan
# msm.form, encode.device, msm.q_waves, msm.q_bg_waves, msm.q_units, bg.eighths, upload.chunks, upload.overlap (options.hpp: the defaults);
# prefer_lds: the generator set's policy flag (gens.hip); shares_chip: a background commit of the context is uncollected (bg_inflight > 0)
DEFAULT_OPTS = {"form": 0, "device_encode": 0, "q_waves": 12, "q_bg_waves": 8, "q_units": 32, "bg_eighths": 5, "upload_chunks": 4, "upload_overlap": 1,
                "prefer_lds": False, "shares_chip": False}
ROLES = ("sync", "begin", "start", "upload")      # msm_launch | sp_commit_rows_dev_begin | _dev_start | _upload_start
FORMS = ("tree1", "tree_fused", "tree_unfused", "windows", "strip", "strip_bg", "flat", "queue", "lds")


def _cdiv(a, b):
    return (a + b - 1) // b


def lds_shape(rows):
    """msm_lds_shape: (row-blocks, rows per workgroup, threads, loader wavefronts)"""
    K = constants()
    b = _cdiv(rows, K["LDS_WG"])
    per = _cdiv(rows, b)
    t = live = _cdiv(per, 64) * 64
    for _ in range(K["LDS_LOADERS"]):
        if t + 64 <= K["LDS_WG"]:
            t += 64
    return b, per, t, (t - live) // 64


def q_cut(launch_rows, ncol, nwin, waves, units_opt, n_cus):
    """msm_q_cut and the workgroup clip of msm_q_enqueue"""
    K = constants()
    workers, ngroups, units = n_cus * waves, _cdiv(launch_rows, 64), ncol * nwin
    share = _cdiv(workers, ngroups)
    ln, recut = units_opt, False
    if ln * share > units:
        ln, recut = _cdiv(units, share), True
    floored = ln < K["Q_MIN_LEN"]
    ln = max(ln, K["Q_MIN_LEN"])
    nb = _cdiv(units, ln)
    S = min(share + K["Q_STEAL"], workers)
    need = _cdiv(nb * ngroups, waves)
    return {"len": ln, "nb": nb, "S": S, "ngroups": ngroups, "share": share, "recut": recut, "len_floored": floored, "S_clamped": share + K["Q_STEAL"] > workers,
            "waves": waves, "wgs": min(n_cus, need), "wgs_clipped": need < n_cus, "last_run_clipped": units % ln != 0}


def plan(rows, cols, blind, nwin, opts, n_cus, flat_slots, lds_nwin=None, role="sync"):
    """what one call runs. nwin: windows of the set's gathered tables; lds_nwin: windows of its LDS-form tables, or None when it has none.
    role: the entry point (ROLES); sync stands for sp_commit_rows, sp_commit_rows_dev, sp_commit_rows_partial and sp_msm_indexed."""
    K = constants()
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    assert role in ROLES and rows >= 1 and cols >= 1
    if role != "sync":
        assert role == "begin" or rows > K["HOST_ENCODE_ROWS"]      # dev_start / upload_start refuse the few-row shapes
    blind = bool(blind) and role != "begin"      # dev_begin takes no blinds
    bg_blocks = n_cus * o["bg_eighths"] // K["BG_DENOM"]
    bg_sub = bg_blocks * K["BG_SUBBLOCKS"] if role == "begin" and bg_blocks > 0 else 0
    shares = bool(o["shares_chip"]) and role != "begin"
    ncol = cols + (1 if blind else 0)
    windowed = rows * ncol * nwin <= (1 << K["WINDOWED_LOG2"])
    # sp_commit_rows_upload_start: the lookups in upload.chunks launches behind the chunks' copies when the rows divide and the commit is not
    # lookup-sized; otherwise copy-then-commit, which is the plan of sp_commit_rows_dev_start
    nch = o["upload_chunks"]
    chunked = role == "upload" and bool(o["upload_overlap"]) and rows % (K["FLAT_ROWS"] * nch) == 0 and not windowed
    launch_rows = rows // nch if chunked else rows
    total = rows * cols
    p = {"rows": rows, "cols": cols, "ncol": ncol, "role": role, "strip": 1, "nstrips": 0, "launch_rows": launch_rows, "nlaunch": nch if chunked else 1, "chunked": chunked, "opt_form": o["form"]}
    form = None
    if windowed:
        P = ncol * nwin
        form = "windows"
    else:
        strip = total // K["TARGET_THREADS"]
        p["strip_floor"] = strip < 1
        strip = max(strip, 1)
        p["strip_over_cols"] = strip > cols
        strip = min(strip, cols)
        nstrips = _cdiv(cols, strip)
        p.update(strip=strip, nstrips=nstrips, last_strip=cols - (nstrips - 1) * strip)
        P = nstrips
        form = "strip"
        if rows % K["FLAT_ROWS"] == 0 and launch_rows % K["FLAT_ROWS"] == 0 and launch_rows // K["FLAT_ROWS"] <= K["FLAT_MAX_BLOCKS"] and not bg_sub and not shares:
            rb, units = launch_rows // K["FLAT_ROWS"], ncol * nwin
            nb = flat_slots // rb
            by_units = nb > units // K["FLAT_MIN_UNITS"]
            if by_units:
                nb = units // K["FLAT_MIN_UNITS"]
            if nb >= 1:
                form, P = "flat", nb
                p.update(flat_rb=rb, flat_by_units=by_units, flat_uneven=units % nb != 0)
        if lds_nwin is not None and (o["form"] == 1 or (o["form"] == 0 and o["prefer_lds"])) and launch_rows >= K["LDS_MIN_ROWS"]:
            slots = bg_sub // K["LDS_BG_DIV"] if bg_sub else (K["LDS_SHARE_MULT"] * n_cus if shares else n_cus)
            nrb, per, thr, loaders = lds_shape(launch_rows)
            units = ncol * lds_nwin
            nb = max(slots // nrb, 1)
            lds_by_units = nb > units // K["LDS_MIN_UNITS"]
            if lds_by_units:
                nb = units // K["LDS_MIN_UNITS"]
            nb = max(nb, 1)
            limit = bg_blocks if role == "begin" and bg_blocks > 0 else 0
            n_wg = nb * nrb
            form, P = "lds", nb
            p.update(nrb=nrb, rows_per_wg=per, threads=thr, loaders=loaders, lds_by_units=lds_by_units, n_wg=n_wg, grid=min(n_wg, limit) if limit else n_wg,
                     grid_limited=bool(limit) and n_wg > limit, lds_xcd=not (bool(limit) and n_wg > limit) and nrb > 1 and n_wg % (8 * nrb) == 0)
        elif o["form"] in (0, 2) and launch_rows >= K["Q_MIN_ROWS"] and launch_rows == rows and _cdiv(rows, K["Q_GROUP"]) <= K["Q_MAX_GROUPS"]:
            cores = bool(bg_sub) or shares
            q = q_cut(launch_rows, ncol, nwin, o["q_bg_waves"] if cores else o["q_waves"], o["q_units"], n_cus)
            form, P = "queue", q["S"]
            p.update(q, coresident=cores)
    chunk, nchunks, two_pass = K["CHUNK"], _cdiv(P, K["CHUNK"]), P > K["TWO_PASS"]
    L = {"windows": 0, "rows": 0, "reduce_pass": 0, "reduce": 0}      # launches per profiling family
    few = rows <= K["HOST_ENCODE_ROWS"]
    small_out = None
    counts = False      # the queue form's slot counts reach the reduction
    if few and windowed:
        nblk = _cdiv(P, K["TREE_BLOCK"])
        form = "tree1" if nblk == 1 else ("tree_unfused" if o["device_encode"] else "tree_fused")
        L["windows"] = 1
        L["reduce"] = (1 if form == "tree_unfused" else 0) + (1 if o["device_encode"] else 0)
        p.update(nblk=nblk, last_block=P - (nblk - 1) * K["TREE_BLOCK"], tree_reduce_strided=nblk > K["TREE_REDUCE"])
        two_pass, encode = False, "batch" if o["device_encode"] else "host"
    else:
        if form == "strip" and role == "begin" and bg_blocks > 0:
            form = "strip_bg"
        L["windows" if windowed else "rows"] = p["nlaunch"]
        counts = form == "queue"      # (also from sp_commit_rows_upload_start: the queue form is planned only for an upload in one chunk)
        if few:
            encode = "batch" if o["device_encode"] else "host"
            batch = bool(o["device_encode"])
        else:
            batch = rows >= K["BATCH_ROWS"]
            encode = "in_reduce"
            if batch:
                encode = "batch_lean" if form == "queue" and p.get("coresident") and role == "begin" else "batch"
            if role == "sync":
                small_out = 32 * rows <= K["HMAP_SIZE"] - K["HMAP_IN"]
        L["reduce_pass"] = 1 if two_pass else 0
        L["reduce"] = 1 + (1 if batch else 0)
        if form in ("strip", "strip_bg"):
            xcd = rows % K["XCD_ROWS"] == 0
            nblocks = _cdiv(p["nstrips"], K["XCD"]) * K["XCD"] * (rows // K["XCD_ROWS"]) if xcd else _cdiv(rows * p["nstrips"], K["STRIP_BLOCK"])
            p.update(xcd=xcd, nblocks=nblocks, xcd_idle=xcd and p["nstrips"] % K["XCD"] != 0, bg_grid=bg_blocks if form == "strip_bg" else 0)
    p.update(form=form, windowed=windowed, P=P, chunk=chunk, nchunks=nchunks, two_pass=two_pass, last_chunk=P - (nchunks - 1) * chunk, encode=encode,
             small_out=small_out, launches=L, counts_in_reduce=counts and not two_pass, counts_in_pass=counts and two_pass,
             reduce_width=(nchunks if two_pass else P) if form not in ("tree1", "tree_fused", "tree_unfused") else p["nblk"])
    return p


def lds_hook_tail(lds_bits, rows):
    """the pieces a wavefront of the LDS form issues after the four hooks of its addition (the `k = 4..npieces` loop of msm_lds_run): 0 whenever
    the workgroup has loader wavefronts (the hooked form then issues nothing)"""
    K = constants()
    _, _, thr, loaders = lds_shape(rows)
    kb = (1 << (lds_bits - 1)) * 96 >> 10
    npieces = _cdiv(kb, thr // 64)
    return 0 if loaders else max(0, npieces - K["LDS_HOOKS"])


def indexed_staging(rows, cols):
    """sp_msm_indexed: True when scalars and indices fit the host-mapped page (the kernel reads them there), False for the device staging buffer"""
    K = constants()
    return 32 * rows * cols + ((4 * cols + 31) & ~31) <= K["HMAP_GEN"]


# ------------------------------------------------------------------ the tiles of the queue form
def live_windows(s, geom):
    """the window at which k_msm_q's ballot finds nothing left of a scalar: the first w with no bit at or above msm_bitpos(w) and no carry
    into w (both stay so for every later window)"""
    carry = 0
    for w in range(geom.nwin):
        if (s >> geom.bitpos(w)) == 0 and carry == 0:
            return w
        carry = 1 if geom.field(s, w) + carry >= geom.half(w) else 0
    return geom.nwin


def group_depths(Z, rows, cols, blind, geom):
    """[group][column] -> max over the group's lanes of live_windows (the blind is column `cols`)"""
    ncol = cols + (1 if blind is not None else 0)
    out = []
    memo = {}

    def lw(s):
        if s not in memo:
            memo[s] = live_windows(s, geom)
        return memo[s]
    for g0 in range(0, rows, 64):
        d = [0] * ncol
        for r in range(g0, min(g0 + 64, rows)):
            for j in range(cols):
                d[j] = max(d[j], lw(Z[r * cols + j]))
            if blind is not None:
                d[cols] = max(d[cols], lw(blind[r]))
        out.append(d)
    return out


def run_tiles(depth, nwin, u, u1):
    """tiles of one run [u, u1) of one group: per column the windows from the run's first one up to the group's depth in that column"""
    n = 0
    j0, j1 = u // nwin, (u1 - 1) // nwin
    for j in range(j0, j1 + 1):
        a = u % nwin if j == j0 else 0
        b = (u1 - 1) % nwin + 1 if j == j1 else nwin
        n += max(0, min(b, depth[j]) - a)
    return n


def issued_tiles(Z, rows, cols, blind, geom, len, order=None):
    """The exact number of tiles k_msm_q issues for the rows x cols matrix Z (canonical integers, row-major; blind: one more scalar per row, or
    None) cut into runs of `len` units: for every 64-row group, every run and every column of the run, the windows from the run's first window
    of that column up to the one at which every lane's remaining scalar and carry are zero. The count depends on (group, run) alone — a run's
    tiles are issued by whichever wavefront draws it from the group's queue, and every wavefront rebuilds the same carries from the same 64
    rows — so it is the same whatever wavefront takes a run, in whatever order (order: a permutation of the (group, run) pairs to count in;
    tests/test_commit_reference.py shuffles it). sp_prof_read_spans reports 64 times this number."""
    depths = group_depths(Z, rows, cols, blind, geom)
    U = (cols + (1 if blind is not None else 0)) * geom.nwin
    nb = _cdiv(U, len)
    items = [(g, bk) for g in range(depths.__len__()) for bk in range(nb)]
    if order is not None:
        assert sorted(order) == items
        items = order
    return sum(run_tiles(depths[g], geom.nwin, bk * len, min((bk + 1) * len, U)) for g, bk in items)


# ------------------------------------------------------------------ tall matrices from a pool of rows
def row_pool_matrix(pool_rows, rows, stride=7):
    """(Z, idx): row r of the rows x cols matrix Z is pool_rows[idx[r]], idx[r] = (r * stride) % len(pool_rows). The pool length is odd, greater
    than 64 and coprime to the stride: consecutive rows are distinct pool rows, a 64-row group holds 64 distinct ones, and the groups of a
    matrix of up to len(pool) groups all begin at different pool rows (no two hold the same arrangement)."""
    n = len(pool_rows)
    assert n % 2 == 1 and n > 64 and math.gcd(n, stride) == 1 and math.gcd(n, 64 * stride) == 1
    idx = [(r * stride) % n for r in range(rows)]
    Z = []
    for i in idx:
        Z += pool_rows[i]
    return Z, idx


def expected(orc, G, H, pool_rows, idx, pool_blinds=None):
    """the commitments of the matrix whose row r is pool_rows[idx[r]] (blind pool_blinds[idx[r]]): ONE orc_commit_rows over the pool, placed.
    G: the compressed generators of the columns; H: the blind's generator (32 bytes)."""
    cols = len(pool_rows[0])
    assert len(G) == 32 * cols and len(H) == 32 and all(len(r) == cols for r in pool_rows)
    n = len(pool_rows)
    out = (ctypes.c_uint8 * (32 * n))()
    flat = [x for r in pool_rows for x in r]
    assert orc.orc_commit_rows(G, sz(cols), H, mont_bulk(flat), sz(n), sz(cols), mont_bulk(pool_blinds) if pool_blinds is not None else None, out) == 0
    out = bytes(out)
    return b"".join(out[32 * i:32 * i + 32] for i in idx)
