"""What an instance's R1CSShapeDigest costs on its two paths (option digest.device): 0 = the entries downloaded, bincode(shape) built and the
sequential deflater run on the host (the path before the device search existed, unchanged); 1 = the stream serialised and tdefl's match search
run on the device, the parser and the Huffman coding on the host behind it. One instance per size, built on the device from an entry list of
about three entries per row and matrix (bench/instance_probe.py's), 2^log2 constraints and variables; the digest is dropped and recomputed.
The two paths are timed ALTERNATELY in one process: 1 warm-up round, then 5 rounds, host clock around Instance.digest() (which ends with the
bytes in hand); median, minimum and maximum of each, and for the device path the median split of its stages and the lookups the match tables
did not answer. The digests of the two paths are compared at every size.
usage: python bench/digest_probe.py [--log2 16 20] [--segment N] [--out profiles/instance_digest.txt]"""
import argparse, ctypes, faulthandler, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "bench"))
faulthandler.dump_traceback_later(1100, exit=True)   # the probe's own time limit

import numpy as np
from spartan_amd import prover as P
from instance_probe import entry_list

WARM, REPS = 1, 5
SPLIT = ("ms_stream", "ms_links", "ms_search_a", "ms_search_b", "ms_download", "ms_wait", "ms_parse")


def median(v):
    return sorted(v)[len(v) // 2]


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
    ts, stats, digests = {0: [], 1: []}, [], {}
    for r in range(WARM + REPS):
        for device in (0, 1):
            ctx.set_option("digest.device", device)
            inst.set_digest(b"")                      # drop the digest: the next use computes it
            t0 = time.perf_counter()
            d = inst.digest()
            dt = (time.perf_counter() - t0) * 1e3
            st = inst.digest_stats()
            assert st["device"] == device
            digests[device] = d
            if r >= WARM:
                ts[device].append(dt)
                if device:
                    stats.append(st)
    assert digests[0] == digests[1], "the two paths disagree at 2^%d" % log2
    n = 24 + 3 * 24 + 48 * total
    lines = ["# 2^%d constraints and variables, %d entries: bincode(shape) %.1f MB, digest %.1f MB, the same bytes on both paths; segments of %d "
             "positions (%d of them); %d alternating rounds after %d warm-up; ms" % (log2, total, n / 1e6, len(digests[0]) / 1e6,
                                                                                    ctx_segment(ctx), int(stats[0]["segments"]), REPS, WARM),
             "%-64s %10s %10s %10s" % ("path", "median", "min", "max")]
    names = {0: "digest.device = 0 (download, host bincode, sequential deflater)", 1: "digest.device = 1 (device stream and match search, host parse)"}
    for device in (0, 1):
        t = sorted(ts[device])
        lines.append("%-64s %10.1f %10.1f %10.1f" % (names[device], median(t), t[0], t[-1]))
    m0, m1 = median(ts[0]), median(ts[1])
    lines.append("host path / device path: %.2fx (medians)" % (m0 / m1))
    lines.append("device path, medians of its stages (host clock: stream build with its wait; device time from events: links, search A, search B, "
                 "downloads; host clock: waiting for the device, parse + block decisions + Huffman coding):")
    lines.append("  " + "  ".join("%s %.1f" % (k[3:], median([s[k] for s in stats])) for k in SPLIT))
    lines.append("  lookups %d, answered by neither table %d (%.3f %%)" % (stats[0]["lookups"], stats[0]["fallbacks"],
                                                                          100.0 * stats[0]["fallbacks"] / max(1, stats[0]["lookups"])))
    inst.free()
    return lines, m1 < m0


def ctx_segment(ctx):
    from spartan_amd.capi import lib
    v = ctypes.c_int64()
    lib.sp_ctx_get_option(ctx.raw(), b"digest.segment", ctypes.byref(v))
    return v.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--segment", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = P.Ctx(0)
    if a.segment:
        ctx.set_option("digest.segment", a.segment)
    lines = ["# python bench/digest_probe.py --log2 %s%s" % (" ".join(str(x) for x in a.log2), " --segment %d" % a.segment if a.segment else "")]
    faster = []
    for log2 in a.log2:
        part, won = run(ctx, log2)
        lines += part + [""]
        faster.append(won)
        print("\n".join(part), flush=True)
    lines.append("device path faster at every size measured: %s" % ("yes" if all(faster) else "no"))
    text = "\n".join(lines) + "\n"
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
