"""What moving tdefl's coder to the device buys an instance's R1CSShapeDigest: digest.device = 1 (device match search, the parser over the
downloaded tables and the coding on the host) and digest.device = 2 (device search and parse, the host codes the tokens), both unchanged,
against digest.device = 3 (block boundaries, histograms, bit emission, stored-block copies and Adler-32 on the device too; the host builds the
Huffman tables and bit offsets per block). The instance is bench/digest_probe.py's: Instance.from_entries over about three entries per row
and matrix, 2^log2 constraints and variables; the digest is dropped and recomputed. The three forms are timed ALTERNATELY in one process: 1
warm-up round, then 5 rounds, host clock around Instance.digest(); median, minimum and maximum of each, and the medians of the stage times.
The keep-or-remove rule: the device coder is kept only if its median is below that of each other form at every size by more than
that form's own min-max spread. The digests of the three forms are compared at every size.
usage: python bench/digest_emit_probe.py [--log2 16 20] [--segment N] [--out profiles/instance_digest_emit.txt]"""
import argparse, ctypes, faulthandler, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))
faulthandler.dump_traceback_later(1100, exit=True)   # the probe's own time limit

import numpy as np
from spartan_amd import prover as P
from instance_probe import entry_list
from digest_probe import ctx_segment, median

WARM, REPS = 1, 5
FORMS = (1, 2, 3)
SPLIT = {1: ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_download", "ms_wait", "ms_parse"),
         2: ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_reach", "ms_emit", "ms_download", "ms_wait", "ms_parse"),
         3: ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_reach", "ms_emit", "ms_blocks", "ms_bits", "ms_wait", "ms_parse", "ms_tables",
             "ms_bytes")}
NAMES = {1: "digest.device = 1 (device search; host parse over tables, coding)", 2: "digest.device = 2 (device search and parse; host codes tokens)",
         3: "digest.device = 3 (device search, parse and coder; host builds tables)"}


def run(ctx, log2):
    nc = nv = 1 << log2
    ni = 10
    rng = np.random.default_rng(log2)
    mats = [entry_list(rng, nc, nv, ni) for _ in range(3)]
    nnz = [len(m[0]) for m in mats]
    total = sum(nnz)
    rows = np.ascontiguousarray(np.concatenate([m[0] for m in mats])); cols = np.ascontiguousarray(np.concatenate([m[1] for m in mats]))
    vals = np.ascontiguousarray(np.concatenate([m[2] for m in mats]))
    inst = P.Instance.from_entries(ctx, nc, nv, ni, nnz, (ctypes.c_uint64 * total).from_buffer(rows), (ctypes.c_uint64 * total).from_buffer(cols),
                                   (ctypes.c_uint8 * (32 * total)).from_buffer(vals))
    ts, stats, digests = {f: [] for f in FORMS}, {f: [] for f in FORMS}, {}
    for r in range(WARM + REPS):
        for form in FORMS:
            ctx.set_option("digest.device", form)
            inst.set_digest(b"")                      # drop the digest: the next use computes it
            t0 = time.perf_counter()
            d = inst.digest()
            dt = (time.perf_counter() - t0) * 1e3
            st = inst.digest_stats()
            assert st["device"] == 1 and st["parse"] == (form >= 2) and st["emit"] == (form == 3)
            digests[form] = d
            if r >= WARM:
                ts[form].append(dt); stats[form].append(st)
    assert digests[1] == digests[2] == digests[3], "the forms disagree at 2^%d" % log2
    n = 24 + 3 * 24 + 48 * total
    lines = ["# 2^%d constraints and variables, %d entries: bincode(shape) %.1f MB, digest %.1f MB, the same bytes in all three forms; segments of %d "
             "positions (%d of them); %d alternating rounds after %d warm-up; ms" % (log2, total, n / 1e6, len(digests[1]) / 1e6, ctx_segment(ctx),
                                                                                    int(stats[1][0]["segments"]), REPS, WARM),
             "%-72s %10s %10s %10s" % ("form", "median", "min", "max")]
    for form in FORMS:
        t = sorted(ts[form])
        lines.append("%-72s %10.1f %10.1f %10.1f" % (NAMES[form], median(t), t[0], t[-1]))
    m3 = median(ts[3])
    won = True
    for form in (1, 2):
        t, m = sorted(ts[form]), median(ts[form])
        spread = t[-1] - t[0]
        ok = m - m3 > spread
        won = won and ok
        lines.append("form %d / form 3: %.2fx (medians); gain %.1f ms against a min-max spread of form %d of %.1f ms: %s"
                     % (form, m / m3, m - m3, form, spread, "kept" if ok else "not kept"))
    lines.append("medians of the stages (host clock: stream, wait, parse = what the host does per segment — parser + coding (form 1), token coder (form 2), "
                 "table building and hand-over (form 3; tables = the table building alone), bytes = the last emission's wait and the download of the "
                 "compressed bytes; device time from events: links, search A, search B, reach, emit = token kernel + compaction, download (forms 1, 2), "
                 "blocks = costs, scan, boundaries, histograms, Adler-32 and the records' copy, bits = the bit emission):")
    for form in FORMS:
        lines.append("  form %d:  " % form + "  ".join("%s %.1f" % (k[3:], median([s[k] for s in stats[form]])) for k in SPLIT[form]))
    s2, s3 = stats[2][0], stats[3][0]
    lines.append("  form 2: %d tokens (%.2f a position), the token coder is %.0f %% of the digest's time; form 3: %d tokens in %d blocks (%d stored, %d "
                 "static), the table building is %.0f %% of the digest's time, %.1f us a block"
                 % (s2["tokens"], s2["tokens"] / n, 100.0 * median([s["ms_parse"] for s in stats[2]]) / median(ts[2]), s3["tokens_coded"], s3["blocks"],
                    s3["stored_blocks"], s3["static_blocks"], 100.0 * median([s["ms_tables"] for s in stats[3]]) / m3,
                    1e3 * median([s["ms_tables"] for s in stats[3]]) / max(1, s3["blocks"])))
    inst.free()
    return lines, won


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = P.Ctx(0)
    if a.segment:
        ctx.set_option("digest.segment", a.segment)
    lines = ["# python bench/digest_emit_probe.py --log2 %s%s" % (" ".join(str(x) for x in a.log2), " --segment %d" % a.segment if a.segment else "")]
    kept = []
    for log2 in a.log2:
        part, won = run(ctx, log2)
        lines += part + [""]
        kept.append(won)
        print("\n".join(part), flush=True)
    lines.append("device coder faster than both other forms at every size measured by more than their spread: %s" % ("yes" if all(kept) else "no"))
    text = "\n".join(lines) + "\n"
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
