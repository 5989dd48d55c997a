"""What moving tdefl's lazy parse to the device buys an instance's R1CSShapeDigest: digest.device = 1 (device match search, the parser over the
downloaded tables and the coding on the host: the path before the device parse existed, unchanged) against digest.device = 2 (device search and
device parse, the host codes the tokens). The instance is bench/digest_probe.py's: Instance.from_entries over about three entries per row and
matrix, 2^log2 constraints and variables; the digest is dropped and recomputed. The two forms are timed ALTERNATELY in one process: 1 warm-up
round, then 5 rounds, host clock around Instance.digest(); median, minimum and maximum of each, and the medians of the stage times of both.
The keep-or-remove rule: the device parse becomes the default only if its median is below the other's at every size by more than
the other's own min-max spread. The digests of the two forms are compared at every size.
usage: python bench/digest_parse_probe.py [--log2 16 20] [--segment N] [--out profiles/instance_digest_parse.txt]"""
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
SPLIT = {1: ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_download", "ms_wait", "ms_parse"),
         2: ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_reach", "ms_emit", "ms_download", "ms_wait", "ms_parse")}
NAMES = {1: "digest.device = 1 (device search; host parse over tables, coding)", 2: "digest.device = 2 (device search and parse; host codes tokens)"}


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
    ts, stats, digests = {1: [], 2: []}, {1: [], 2: []}, {}
    for r in range(WARM + REPS):
        for form in (1, 2):
            ctx.set_option("digest.device", form)
            inst.set_digest(b"")                      # drop the digest: the next use computes it
            t0 = time.perf_counter()
            d = inst.digest()
            dt = (time.perf_counter() - t0) * 1e3
            st = inst.digest_stats()
            assert st["device"] == 1 and st["parse"] == (form == 2)
            digests[form] = d
            if r >= WARM:
                ts[form].append(dt); stats[form].append(st)
    assert digests[1] == digests[2], "the two forms disagree at 2^%d" % log2
    n = 24 + 3 * 24 + 48 * total
    lines = ["# 2^%d constraints and variables, %d entries: bincode(shape) %.1f MB, digest %.1f MB, the same bytes in both forms; segments of %d "
             "positions (%d of them); %d alternating rounds after %d warm-up; ms" % (log2, total, n / 1e6, len(digests[1]) / 1e6, ctx_segment(ctx),
                                                                                    int(stats[1][0]["segments"]), REPS, WARM),
             "%-68s %10s %10s %10s" % ("form", "median", "min", "max")]
    for form in (1, 2):
        t = sorted(ts[form])
        lines.append("%-68s %10.1f %10.1f %10.1f" % (NAMES[form], median(t), t[0], t[-1]))
    t1, m1, m2 = sorted(ts[1]), median(ts[1]), median(ts[2])
    spread = t1[-1] - t1[0]
    won = m1 - m2 > spread
    lines.append("host parse / device parse: %.2fx (medians); gain %.1f ms against a min-max spread of the host-parse form of %.1f ms: %s"
                 % (m1 / m2, m1 - m2, spread, "kept" if won else "not kept"))
    lines.append("medians of the stages (host clock: stream, wait, parse = the host's parser + coding (form 1) or token coder alone (form 2); device "
                 "time from events: links, search A, search B, reach = jumps, exits, entries and marks, emit = token kernel + compaction, download):")
    for form in (1, 2):
        lines.append("  form %d:  " % form + "  ".join("%s %.1f" % (k[3:], median([s[k] for s in stats[form]])) for k in SPLIT[form]))
    s1, s2 = stats[1][0], stats[2][0]
    lines.append("  form 1: %d look-ups on the host, %d answered by neither table; form 2: %d tokens (%.2f a position), %d look-ups searched on the spot "
                 "by the device" % (s1["lookups"], s1["fallbacks"], s2["tokens"], s2["tokens"] / n, s2["device_fallbacks"]))
    lines.append("  form 2: the token coder is %.0f %% of the digest's time" % (100.0 * median([s["ms_parse"] for s in stats[2]]) / m2))
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
    lines = ["# python bench/digest_parse_probe.py --log2 %s%s" % (" ".join(str(x) for x in a.log2), " --segment %d" % a.segment if a.segment else "")]
    kept = []
    for log2 in a.log2:
        part, won = run(ctx, log2)
        lines += part + [""]
        kept.append(won)
        print("\n".join(part), flush=True)
    lines.append("device parse faster at every size measured by more than the spread: %s" % ("yes" if all(kept) else "no"))
    text = "\n".join(lines) + "\n"
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
