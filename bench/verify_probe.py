"""What NIZK::verify and SNARK::verify cost on the device (spartan_amd/host/verifier.cc) next to the oracle's restated verifier on the host cores of the same
box. One process, its own time limit, stops at the first step that fails. Per size (2^16, 2^20, 2^22 constraints, synthetic instances):
  (a) NIZK.verify of the HIP prover's proof, warm (digest set, generator tables built, one verification done): median of 20 calls timed with
      the host clock — the call ends in a wait for the device, so the wall time is the verification;
  (b) the msm_var kernel chain of one verification (sp_prof_*, HIP events; collected in runs of their own, not in the timed ones) and the
      round trips of one verification (sp_ctx_trips);
  (c) the oracle's orc_nizk_verify_bytes on the same bytes, 16 host threads, median of 3.
The reference publishes 414.5 ms for NIZK::verify at 2^20 on its own machine: context, not a comparison on this box.
--what snark: the same three for SNARK.verify against a Commitment loaded from bincode bytes (two of its four C_LZ go through sp_msm_var, two
through the resident point sets of the commitment, sp_msm_points) and the oracle's orc_snark_verify_bytes.
--what msm: sp_msm_points against sp_msm_var on identical points and scalars (n = 2048, 4096), the calls interleaved in one process, 20 samples
each after 3 warm pairs: median and spread (min .. max) per call, the table build (sp_points_upload) beside them.
--what snark_many --batch 1,4,16,64: SNARK.verify_many of K proofs of one circuit (lock step: spartan_amd/host/batch_gate.hpp) against K sequential
SNARK.verify calls on the same proofs, the two interleaved sample by sample in one process: ms per batch and per proof, round trips, and the
device time of the two variable-base MSM families per launch chain.
--what nizk_many --batch 1,4,16,64: the same for NIZK.verify_many against K sequential NIZK.verify calls, with the device time of the batched
evaluation (one `sparse` record a batch: sp_sparse_evaluate_many_begin) beside K times the single call's, and the keep-or-drop rule of DESIGN.md
section 3 applied at K = 16: the per-proof medians must differ by more than the spread (max - min) of the samples.
--gens prover|verifier (--what nizk, snark): which generators the timed verifications are handed — the prover's (fixed-base window tables; the
proof is always made under them) or verifier-only ones (SNARKGens.verifier_only / NIZKGens.verifier_only: the streams as resident point sets).
--what gens: both kinds in ONE session (profiles/verifier_gens.txt), per size: creation time and bytes held of either kind, and NIZK.verify /
SNARK.verify of one proof under either, the two interleaved sample by sample, median of 20 after 3 warm pairs. The yardstick is the prover's.
--what encode: obtaining the circuit's commitment, both ways in ONE session (profiles/verifier_encode.txt), per size: SNARKGens.verifier_only +
Commitment.encode (sp_commit_rows_points over the resident sets) against SNARKGens(...) + SNARK.encode (window tables): time of each step on
the host clock, peak HBM above the session's baseline while it runs (free device memory polled from a second thread) and HBM held afterwards,
then the encode call alone, warm (median of 3), and the HIP-event time of its commit_rows_points launch chains. --kernel-stats FILE adds the
kernels' own times from the kernel statistics (csv) of a SEPARATE profiler run of `--what encode --kernel-run` (the verifier's path alone, once).
usage: python bench/verify_probe.py [--what nizk|snark|msm|snark_many|nizk_many|gens|encode] [--gens prover|verifier] [--out profiles/nizk_verify.txt]
       [--sizes 16,20,22] [--batch 1,4,16,64] [--kernel-run] [--kernel-stats FILE]"""
import argparse, ctypes, faulthandler, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
faulthandler.dump_traceback_later(900, exit=True)   # the probe's own time limit

from spartan_amd import capi, prover as P
from tests.helpers import load_oracle, sz, vp

WARM, REPS = 3, 20
L = capi.lib
LABEL = b"nizk_example"


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def median_ms(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def family(raw, name):
    cap = 64
    names = (ctypes.c_char_p * cap)(); ms = (ctypes.c_double * cap)(); n = (ctypes.c_uint64 * cap)(); by = (ctypes.c_double * cap)()
    k = L.sp_prof_read(raw, names, ms, n, by, ctypes.c_int(cap))
    return {names[i].decode(): (ms[i], int(n[i])) for i in range(k)}.get(name, (0.0, 0))


def comm_parts(cb):
    """the six numbers and the two share vectors of bincode(ComputationCommitment), as orc_snark_verify_bytes takes them"""
    h = [int.from_bytes(cb[8 * i:8 * i + 8], "little") for i in range(6)]
    n_ops = int.from_bytes(cb[48:56], "little")
    o = 56 + 32 * n_ops
    n_mem = int.from_bytes(cb[o:o + 8], "little")
    return h, cb[56:o], cb[o + 8:o + 8 + 32 * n_mem]


def gens_kind(args):
    return "verifier-only (resident point sets; G_hat through sp_msm_points_range)" if args.gens == "verifier" else "the prover's (G_hat through sp_commit_rows)"


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def pair_medians(a, b):
    """the two calls interleaved sample by sample: WARM warm pairs, then REPS samples each -> ((median, min, max) of a, of b)"""
    ta, tb = [], []
    for i in range(WARM + REPS):
        _, x = timed(a)
        _, y = timed(b)
        if i >= WARM:
            ta.append(x); tb.append(y)
    ta.sort(); tb.sort()
    return (ta[len(ta) // 2], ta[0], ta[-1]), (tb[len(tb) // 2], tb[0], tb[-1])


def gens_session(args, orc):
    """both kinds of generators in one session: what each costs to make and to hold, and what a verification costs under each"""
    label = b"snark_example"
    lines = ["Verifier-only generators against the prover's, one session (bench/verify_probe.py --what gens; host CPU: %s)" % cpu_model(),
             "creation: host clock around the constructor, the prover's first (nothing of the size resident), then the verifier-only ones; bytes: HBM held by",
             "the generator tables; verify: one proof under either kind, the two calls interleaved, %d warm pairs then %d samples each, median (min, max)" % (WARM, REPS),
             ""]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    GiB = float(1 << 30)
    row = lambda what, full, light: "  %-14s prover's %s   verifier-only %s" % (what, full, light)
    stat = lambda m: "%9.3f ms (%.3f, %.3f)" % m
    for s in [int(x) for x in args.sizes.split(",")]:
        N, ni, seed = 1 << s, 10, s
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        inst.set_digest(b"digest-%d" % s)
        # NIZK: one stream
        ng, ng_ms = timed(lambda: P.NIZKGens(ctx, N, N, ni))
        nv, nv_ms = timed(lambda: P.NIZKGens.verifier_only(ctx, N, N, ni))
        proof = P.NIZK.prove(ctx, inst, inst.vars, inst.inputs, ng, LABEL, P.seed_scalar(b"tape", seed))
        full = lambda: P.NIZK.verify_status(ctx, inst, proof, inst.inputs, ng, LABEL)
        light = lambda: P.NIZK.verify_status(ctx, inst, proof, inst.inputs, nv, LABEL)
        if full() != 1 or light() != 1:
            raise SystemExit("2^%d: a NIZK verification rejected the prover's proof" % s)
        mf, ml = pair_medians(full, light)
        t0 = L.sp_ctx_trips(raw); light(); trips = L.sp_ctx_trips(raw) - t0
        lines += ["synthetic 2^%d, NIZK: proof %d bytes, %d round trips per verification under verifier-only generators" % (s, len(proof), trips),
                  row("creation", "%9.1f ms" % ng_ms, "%9.1f ms" % nv_ms),
                  row("bytes held", "%9.3f GiB" % (ng.resident_bytes() / GiB), "%9.3f GiB" % (nv.resident_bytes() / GiB)),
                  row("NIZK.verify", stat(mf), stat(ml))]
        print("\n".join(lines[-4:]), flush=True)
        nv.free(); ng.free()
        # SNARK: two streams (the prover's tables of the first were freed with the NIZK generators: built again here)
        sg, sg_ms = timed(lambda: P.SNARKGens(ctx, N, N, ni, N))
        sv, sv_ms = timed(lambda: P.SNARKGens.verifier_only(ctx, N, N, ni, N))
        enc = P.SNARK.encode(ctx, inst, sg)
        proof = P.SNARK.prove(ctx, inst, enc, inst.vars, inst.inputs, sg, label, P.seed_scalar(b"tape", seed))
        comm = P.Commitment.load(ctx, enc.serialize_commitment())
        full = lambda: P.SNARK.verify_status(ctx, comm, proof, inst.inputs, sg, label)
        light = lambda: P.SNARK.verify_status(ctx, comm, proof, inst.inputs, sv, label)
        if full() != 1 or light() != 1:
            raise SystemExit("2^%d: a SNARK verification rejected the prover's proof" % s)
        mf, ml = pair_medians(full, light)
        t0 = L.sp_ctx_trips(raw); light(); trips = L.sp_ctx_trips(raw) - t0
        lines += ["synthetic 2^%d, SNARK: proof %d bytes, generator streams of %d + %d points, %d round trips per verification under verifier-only generators" % (
                      s, len(proof), len(sv.stream(0)) // 32, len(sv.stream(1)) // 32, trips),
                  row("creation", "%9.1f ms" % sg_ms, "%9.1f ms" % sv_ms),
                  row("bytes held", "%9.3f GiB" % (sg.resident_bytes() / GiB), "%9.3f GiB" % (sv.resident_bytes() / GiB)),
                  row("SNARK.verify", stat(mf), stat(ml))]
        print("\n".join(lines[-4:]), flush=True)
        comm.free(); enc.free(); sv.free(); sg.free(); inst.free()
    ctx.close()
    return lines


class PeakHBM:
    """device memory in use above `base` while the block runs: free memory polled every millisecond from a second thread"""
    def __init__(self, base):
        import threading, torch
        self.base, self.low, self.stop, self.torch = base, base, False, torch
        self.th = threading.Thread(target=self.poll, daemon=True)

    def poll(self):
        while not self.stop:
            self.low = min(self.low, self.torch.cuda.mem_get_info(0)[0])
            time.sleep(0.001)

    def __enter__(self):
        self.th.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        self.th.join()
        self.low = min(self.low, self.torch.cuda.mem_get_info(0)[0])
        self.peak = self.base - self.low
        self.held = self.base - self.torch.cuda.mem_get_info(0)[0]


def kernel_stats_lines(path):
    """the k_rowp_* rows of a profiler's kernel statistics csv (columns Name, Calls, TotalDurationNs, AverageNs, MinNs, MaxNs)"""
    import csv
    out = []
    for row in csv.DictReader(open(path)):
        name = row.get("Name") or row.get("KernelName") or ""
        if "k_rowp_" in name:
            short = "k_rowp_sum" if "k_rowp_sum" in name else "k_rowp_finish"
            out.append("  %-14s calls %s, total %.3f ms, average %.3f ms (min %.3f, max %.3f)" % (
                short, row["Calls"], float(row["TotalDurationNs"]) / 1e6, float(row["AverageNs"]) / 1e6, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6))
    return out


def encode_session(args, orc):
    """the commitment of a circuit, obtained by a verifier (verifier-only generators, Commitment.encode) and by a prover (SNARKGens, SNARK.encode)"""
    import torch
    sizes = [int(x) for x in args.sizes.split(",")]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    if args.kernel_run:       # under a profiler: the verifier's path alone, once a size (two launch chains: comb_ops, comb_mem)
        for s in sizes:
            N, ni = 1 << s, 10
            inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=s)
            sv = P.SNARKGens.verifier_only(ctx, N, N, ni, N)
            h = P.Commitment.encode(ctx, inst, sv)
            print("2^%d: commitment of %d bytes" % (s, len(h.serialize())), flush=True)
            h.free(); sv.free(); inst.free()
        ctx.close()
        return ["kernel run done"]
    lines = ["The commitment of a circuit without the prover's tables (bench/verify_probe.py --what encode; host CPU: %s)" % cpu_model(),
             "one session, warm (both paths run once at 2^10 first); per step: host clock around the call; peak: HBM in use above the baseline of the size while",
             "the two steps run (free memory polled each ms); held: above the baseline once both have returned; `again`: the encode call alone, %d more times, median (min, max)" % 3,
             ""]
    GiB = float(1 << 30)

    def warm():
        inst = P.Instance.produce_synthetic_r1cs(ctx, 1024, 1024, 10, seed=1)
        sv = P.SNARKGens.verifier_only(ctx, 1024, 1024, 10, 1024); sg = P.SNARKGens(ctx, 1024, 1024, 10, 1024)
        h = P.Commitment.encode(ctx, inst, sv); e = P.SNARK.encode(ctx, inst, sg)
        assert h.serialize() == e.serialize_commitment()
        e.free(); h.free(); sg.free(); sv.free(); inst.free()
    warm()
    torch.cuda.synchronize()
    stat = lambda m: "%9.3f ms (%.3f, %.3f)" % m
    for s in sizes:
        N, ni = 1 << s, 10
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=s)
        L.sp_ctx_sync(raw)
        base = torch.cuda.mem_get_info(0)[0]
        with PeakHBM(base) as v:
            sv, sv_ms = timed(lambda: P.SNARKGens.verifier_only(ctx, N, N, ni, N))
            h, h_ms = timed(lambda: P.Commitment.encode(ctx, inst, sv))
        cb = h.serialize()
        again_v = median_ms(lambda: P.Commitment.encode(ctx, inst, sv).free(), 0, 3)
        L.sp_prof_enable(raw, ctypes.c_int(1)); L.sp_prof_reset(raw)
        P.Commitment.encode(ctx, inst, sv).free()
        cp_ms, cp_n = family(raw, "commit_rows_points")
        L.sp_prof_enable(raw, ctypes.c_int(0))
        _, ops, mem = comm_parts(cb)
        h.free(); sv.free()
        L.sp_ctx_sync(raw)
        with PeakHBM(base) as p:
            sg, sg_ms = timed(lambda: P.SNARKGens(ctx, N, N, ni, N))
            enc, enc_ms = timed(lambda: P.SNARK.encode(ctx, inst, sg))
        if enc.serialize_commitment() != cb:
            raise SystemExit("2^%d: the two commitments differ" % s)
        enc.free()
        again_p = median_ms(lambda: P.SNARK.encode(ctx, inst, sg).free(), 0, 3)
        lines += ["synthetic 2^%d: commitment of %d + %d shares, %d bytes, the same either way" % (s, len(ops) // 32, len(mem) // 32, len(cb)),
                  "  verifier: SNARKGens.verifier_only %9.1f ms + Commitment.encode %9.1f ms = %9.1f ms; peak %8.3f GiB, held %8.3f GiB" % (
                      sv_ms, h_ms, sv_ms + h_ms, v.peak / GiB, v.held / GiB),
                  "  prover:   SNARKGens               %9.1f ms + SNARK.encode      %9.1f ms = %9.1f ms; peak %8.3f GiB, held %8.3f GiB (the decommitment included)" % (
                      sg_ms, enc_ms, sg_ms + enc_ms, p.peak / GiB, p.held / GiB),
                  "  again:    Commitment.encode %s; SNARK.encode %s" % (stat(again_v), stat(again_p)),
                  "  commit_rows_points launch chains (HIP events, a run of its own): %d, %.3f ms in all" % (cp_n, cp_ms)]
        print("\n".join(lines[-5:]), flush=True)
        sg.free(); inst.free()
    ctx.close()
    if args.kernel_stats:
        lines += ["", "kernels of the verifier's path, from the kernel statistics of a separate profiler run (--kernel-run, sizes %s, one Commitment.encode each):" % args.sizes]
        lines += kernel_stats_lines(args.kernel_stats) or ["  (no k_rowp_* row in %s)" % os.path.basename(args.kernel_stats)]
    return lines


def snark(args, orc):
    label = b"snark_example"
    lines = ["SNARK::verify on the device against the oracle's verifier on the host (bench/verify_probe.py --what snark; host CPU: %s)" % cpu_model(),
             "(a): median of %d warm calls, host clock; msm_var / msm_points: HIP events around their launch chains, runs of their own; (c): median of 3, 16 threads" % REPS,
             "generators of the timed verifications: %s" % gens_kind(args),
             ""]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    for s in [int(x) for x in args.sizes.split(",")]:
        N, ni, seed = 1 << s, 10, s
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        gens = P.SNARKGens(ctx, N, N, ni, N)
        enc = P.SNARK.encode(ctx, inst, gens)
        proof = P.SNARK.prove(ctx, inst, enc, inst.vars, inst.inputs, gens, label, P.seed_scalar(b"tape", seed))
        cb = enc.serialize_commitment()
        t0 = time.perf_counter(); comm = P.Commitment.load(ctx, cb); load_ms = (time.perf_counter() - t0) * 1e3
        vgens = P.SNARKGens.verifier_only(ctx, N, N, ni, N) if args.gens == "verifier" else gens
        verify = lambda: P.SNARK.verify_status(ctx, comm, proof, inst.inputs, vgens, label)
        if verify() != 1:
            raise SystemExit("2^%d: the device verifier rejected the prover's proof" % s)
        med, lo, hi = median_ms(verify, WARM, REPS)
        t0 = L.sp_ctx_trips(raw); verify(); trips = L.sp_ctx_trips(raw) - t0
        L.sp_prof_enable(raw, ctypes.c_int(1)); L.sp_prof_reset(raw)
        for _ in range(5):
            verify()
        mv_ms, mv_n = family(raw, "msm_var")
        mp_ms, mp_n = family(raw, "msm_points")
        if vgens is not gens:
            vgens.free()
        L.sp_prof_enable(raw, ctypes.c_int(0))
        h, ops, mem = comm_parts(cb)
        og = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(ni), sz(N)))
        overify = lambda: orc.orc_snark_verify_bytes(proof, sz(len(proof)), og, sz(h[0]), sz(h[1]), sz(h[2]), sz(h[4]), sz(h[5]), ops, sz(len(ops) // 32), mem,
                                                     sz(len(mem) // 32), inst.inputs, label)
        if overify() != 1:
            raise SystemExit("2^%d: the oracle rejected the prover's proof" % s)
        omed, olo, ohi = median_ms(overify, 0, 3)
        orc.orc_snark_gens_free(og)
        lines += ["synthetic 2^%d: proof %d bytes, commitment %d + %d shares (loaded once in %.1f ms), %d round trips per verification" % (
                      s, len(proof), len(ops) // 32, len(mem) // 32, load_ms, trips),
                  "  (a) SNARK.verify, device                 median %9.3f ms   (min %.3f, max %.3f)" % (med, lo, hi),
                  "  (b) msm_var launch chain                 mean   %9.3f ms   (of %d); msm_points launch chain mean %.3f ms (of %d)" % (
                      mv_ms / max(mv_n, 1), mv_n, mp_ms / max(mp_n, 1), mp_n),
                  "  (c) oracle orc_snark_verify_bytes        median %9.3f ms   (min %.3f, max %.3f)" % (omed, olo, ohi),
                  "  (c) / (a) = %.1f" % (omed / med)]
        print("\n".join(lines[-5:]), flush=True)
        comm.free(); enc.free(); gens.free(); inst.free()
    ctx.close()
    return lines


def snark_many(args, orc):
    label = b"snark_example"
    DISTINCT = 4
    lines = ["SNARK::verify_many (K proofs of one circuit in lock step) against K sequential SNARK::verify calls (bench/verify_probe.py --what snark_many; "
             "host CPU: %s, %d CPUs for this process)" % (cpu_model(), len(os.sched_getaffinity(0))),
             "per K: %d warm pairs, then %d samples of (one verify_many, K verify calls) interleaved on the host clock, medians; a batch holds %d distinct "
             "proofs (tape seeds) in rotation; msm_var / msm_points: HIP events around their launch chains, runs of their own" % (WARM, REPS, DISTINCT),
             ""]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    med = lambda ts: sorted(ts)[len(ts) // 2]
    for s in [int(x) for x in args.sizes.split(",")]:
        N, ni, seed = 1 << s, 10, s
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        gens = P.SNARKGens(ctx, N, N, ni, N)
        enc = P.SNARK.encode(ctx, inst, gens)
        distinct = [P.SNARK.prove(ctx, inst, enc, inst.vars, inst.inputs, gens, label, P.seed_scalar(b"tape", seed + 100 * i)) for i in range(DISTINCT)]
        comm = P.Commitment.load(ctx, enc.serialize_commitment())
        single = lambda p: P.SNARK.verify_status(ctx, comm, p, inst.inputs, gens, label)
        lines.append("synthetic 2^%d: proof %d bytes" % (s, len(distinct[0])))
        print(lines[-1], flush=True)
        for K in [int(x) for x in args.batch.split(",")]:
            batch = [distinct[i % DISTINCT] for i in range(K)]
            many = lambda: P.SNARK.verify_many(ctx, comm, batch, inst.inputs, gens, label)
            seq = lambda: [single(p) for p in batch]
            if many() != [1] * K or seq() != [1] * K:
                raise SystemExit("2^%d, K = %d: a proof of the prover was not accepted" % (s, K))
            tm, ts = [], []
            for i in range(WARM + REPS):
                t0 = time.perf_counter(); many(); t1 = time.perf_counter(); seq(); t2 = time.perf_counter()
                if i >= WARM:
                    tm.append((t1 - t0) * 1e3); ts.append((t2 - t1) * 1e3)
            t0 = L.sp_ctx_trips(raw); many(); trips_m = L.sp_ctx_trips(raw) - t0
            t0 = L.sp_ctx_trips(raw); seq(); trips_s = L.sp_ctx_trips(raw) - t0
            fam = {}
            for name, fn in (("many", many), ("seq", seq)):
                L.sp_prof_enable(raw, ctypes.c_int(1)); L.sp_prof_reset(raw)
                for _ in range(3):
                    fn()
                fam[name] = (family(raw, "msm_var"), family(raw, "msm_points"))
                L.sp_prof_enable(raw, ctypes.c_int(0))
            chain = lambda f: "%.3f ms (of %d)" % (f[0] / max(f[1], 1), f[1])
            mm, sm = med(tm), med(ts)
            lines += ["  K = %2d  verify_many   median %9.3f ms a batch = %8.3f ms a proof   (min %.3f, max %.3f), %d round trips a batch" % (
                          K, mm, mm / K, min(tm), max(tm), trips_m),
                      "          K x verify    median %9.3f ms         = %8.3f ms a proof   (min %.3f, max %.3f), %d round trips" % (
                          sm, sm / K, min(ts), max(ts), trips_s),
                      "          launch chains: verify_many msm_var %s, msm_points %s; verify msm_var %s, msm_points %s" % (
                          chain(fam["many"][0]), chain(fam["many"][1]), chain(fam["seq"][0]), chain(fam["seq"][1])),
                      "          sequential / batched = %.2f per proof%s" % (sm / mm, "" if sm >= mm else "   (the batch is SLOWER per proof)")]
            print("\n".join(lines[-4:]), flush=True)
        comm.free(); enc.free(); gens.free(); inst.free()
    ctx.close()
    return lines


def nizk_many(args, orc):
    DISTINCT = 4
    lines = ["NIZK::verify_many (K proofs of one instance in lock step) against K sequential NIZK::verify calls (bench/verify_probe.py --what nizk_many; "
             "host CPU: %s, %d CPUs for this process)" % (cpu_model(), len(os.sched_getaffinity(0))),
             "per K: %d warm pairs, then %d samples of (one verify_many, K verify calls) interleaved on the host clock, medians; a batch holds %d distinct "
             "proofs (tape seeds) in rotation; sparse / eq_expand: HIP events around their launches, runs of their own (3 each)" % (WARM, REPS, DISTINCT),
             "rule (DESIGN.md section 3): the batch is kept if at K = 16 its per-proof median lies below the sequential one by more than the spread (max - min) of the samples",
             ""]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    med = lambda ts: sorted(ts)[len(ts) // 2]
    for s in [int(x) for x in args.sizes.split(",")]:
        N, ni, seed = 1 << s, 10, s
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        inst.set_digest(b"digest-%d" % s)
        gens = P.NIZKGens(ctx, N, N, ni)
        distinct = [P.NIZK.prove(ctx, inst, inst.vars, inst.inputs, gens, LABEL, P.seed_scalar(b"tape", seed + 100 * i)) for i in range(DISTINCT)]
        single = lambda p: P.NIZK.verify_status(ctx, inst, p, inst.inputs, gens, LABEL)
        lines.append("synthetic 2^%d: proof %d bytes" % (s, len(distinct[0])))
        print(lines[-1], flush=True)
        for K in [int(x) for x in args.batch.split(",")]:
            batch = [distinct[i % DISTINCT] for i in range(K)]
            many = lambda: P.NIZK.verify_many(ctx, inst, batch, inst.inputs, gens, LABEL)
            seq = lambda: [single(p) for p in batch]
            if many() != [1] * K or seq() != [1] * K:
                raise SystemExit("2^%d, K = %d: a proof of the prover was not accepted" % (s, K))
            tm, ts = [], []
            for i in range(WARM + REPS):
                t0 = time.perf_counter(); many(); t1 = time.perf_counter(); seq(); t2 = time.perf_counter()
                if i >= WARM:
                    tm.append((t1 - t0) * 1e3); ts.append((t2 - t1) * 1e3)
            t0 = L.sp_ctx_trips(raw); many(); trips_m = L.sp_ctx_trips(raw) - t0
            t0 = L.sp_ctx_trips(raw); seq(); trips_s = L.sp_ctx_trips(raw) - t0
            fam = {}
            for name, fn in (("many", many), ("seq", seq)):
                L.sp_prof_enable(raw, ctypes.c_int(1)); L.sp_prof_reset(raw)
                for _ in range(3):
                    fn()
                fam[name] = (family(raw, "sparse"), family(raw, "eq_expand"))
                L.sp_prof_enable(raw, ctypes.c_int(0))
            mm, sm = med(tm), med(ts)
            (bs_ms, bs_n), (be_ms, be_n) = fam["many"]
            (ss_ms, ss_n), (se_ms, se_n) = fam["seq"]
            one_sparse, one_eq = ss_ms / max(ss_n, 1), se_ms / max(se_n, 1)
            lines += ["  K = %2d  verify_many   median %9.3f ms a batch = %8.3f ms a proof   (min %.3f, max %.3f), %d round trips a batch" % (
                          K, mm, mm / K, min(tm), max(tm), trips_m),
                      "          K x verify    median %9.3f ms         = %8.3f ms a proof   (min %.3f, max %.3f), %d round trips" % (
                          sm, sm / K, min(ts), max(ts), trips_s),
                      "          evaluation: batched sparse %.3f ms a batch (%d record a batch, %d eq_expand); single call sparse %.3f ms + 2 eq_expand of %.3f ms: K x = %.3f ms (+ %.3f)" % (
                          bs_ms / 3, bs_n // 3, be_n // 3, one_sparse, one_eq, K * one_sparse, 2 * K * one_eq),
                      "          sequential / batched = %.2f per proof%s" % (sm / mm, "" if sm >= mm else "   (the batch is SLOWER per proof)")]
            if K == 16:
                spread = max(max(tm) - min(tm), max(ts) - min(ts)) / K
                gain = (sm - mm) / K
                lines.append("          rule at K = 16: gain %.3f ms a proof, widest spread of the %d samples %.3f ms a proof: %s" % (
                    gain, REPS, spread, "KEPT (a gain beyond the spread)" if gain > spread else "NOT kept by the rule (no gain beyond the spread)"))
            print("\n".join(lines[-(5 if K == 16 else 4):]), flush=True)
        gens.free(); inst.free()
    ctx.close()
    return lines


def msm(args, orc):
    import random
    from tests import msm_var_cases as M
    from tests.helpers import mont_bulk, fast_scalars
    lines = ["sp_msm_points (resident point set) against sp_msm_var on identical points and scalars (bench/verify_probe.py --what msm)",
             "calls interleaved in one process, %d warm pairs, then %d samples each on the host clock (a call ends in its wait for the device)" % (WARM, REPS),
             ""]
    ctx = capi.Ctx(0)
    out = (ctypes.c_uint8 * 32)()
    for n in (2048, 4096):
        pts = b"".join(M.points(orc, n))
        S = mont_bulk(fast_scalars(random.Random(n), n))
        h = vp()
        t0 = time.perf_counter()
        rc = L.sp_points_upload(ctx.h, pts, sz(n), ctypes.byref(h))
        build_ms = (time.perf_counter() - t0) * 1e3
        if rc != 0:
            raise SystemExit("sp_points_upload: %d" % rc)
        tv, tp, rv, rp = [], [], None, None
        for i in range(WARM + REPS):
            t0 = time.perf_counter(); rc1 = L.sp_msm_var(ctx.h, pts, S, sz(n), out); t1 = time.perf_counter(); rv = bytes(out)
            rc2 = L.sp_msm_points(ctx.h, h, S, sz(n), out); t2 = time.perf_counter(); rp = bytes(out)
            if rc1 != 0 or rc2 != 0 or rv != rp:
                raise SystemExit("n = %d: the two multiplications disagree (%d, %d)" % (n, rc1, rc2))
            if i >= WARM:
                tv.append((t1 - t0) * 1e3); tp.append((t2 - t1) * 1e3)
        L.sp_points_free(h)
        tv.sort(); tp.sort()
        mv, mp = tv[len(tv) // 2], tp[len(tp) // 2]
        spread = max(tv[-1] - tv[0], tp[-1] - tp[0])
        lines += ["n = %d: table build (sp_points_upload, %d MiB) %.2f ms, once" % (n, n * 64 // 1024, build_ms),
                  "  sp_msm_var     median %8.3f ms   (min %.3f, max %.3f)" % (mv, tv[0], tv[-1]),
                  "  sp_msm_points  median %8.3f ms   (min %.3f, max %.3f)" % (mp, tp[0], tp[-1]),
                  "  difference of the medians %.3f ms, widest spread of the %d samples %.3f ms: %s" % (
                      mv - mp, REPS, spread, "a gain beyond the spread" if mv - mp > spread else "NO gain beyond the spread")]
        print("\n".join(lines[-4:]), flush=True)
    ctx.close()
    return lines


def finish(args, lines):
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=None, help="log2 sizes; default 16,20,22 (nizk_many: 16,20)")
    ap.add_argument("--what", default="nizk", choices=["nizk", "snark", "msm", "snark_many", "nizk_many", "gens", "encode"])
    ap.add_argument("--gens", default="prover", choices=["prover", "verifier"], help="--what nizk / snark: the generators the timed verifications take")
    ap.add_argument("--batch", default="1,4,16,64", help="--what snark_many / nizk_many: the batch sizes K")
    ap.add_argument("--kernel-run", action="store_true", help="--what encode: the verifier's path alone, once a size (the run a profiler wraps)")
    ap.add_argument("--kernel-stats", default=None, help="--what encode: kernel statistics csv of such a run, quoted in the output")
    args = ap.parse_args()
    if args.sizes is None:
        args.sizes = "16,20" if args.what in ("nizk_many", "gens", "encode") else "16,20,22"
    orc = load_oracle()
    orc.orc_set_threads(ctypes.c_int(16))
    if args.what != "nizk":
        return finish(args, {"snark": snark, "msm": msm, "snark_many": snark_many, "nizk_many": nizk_many, "gens": gens_session, "encode": encode_session}[args.what](args, orc))
    lines = ["NIZK::verify on the device against the oracle's verifier on the host (bench/verify_probe.py; host CPU: %s)" % cpu_model(),
             "(a): median of %d warm calls, host clock; msm_var: HIP events around its launch chain, runs of their own; (c): median of 3, 16 threads" % REPS,
             "generators of the timed verifications: %s" % gens_kind(args),
             ""]
    ctx = P.Ctx(0)
    raw = ctx.raw()
    for s in [int(x) for x in args.sizes.split(",")]:
        N, ni, seed = 1 << s, 10, s
        digest = b"digest-%d" % s           # the deflate of the shape (seconds at 2^20) is setup, as in Instance::new of the reference
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
        inst.set_digest(digest)
        gens = P.NIZKGens(ctx, N, N, ni)
        proof = P.NIZK.prove(ctx, inst, inst.vars, inst.inputs, gens, LABEL, P.seed_scalar(b"tape", seed))
        vgens = P.NIZKGens.verifier_only(ctx, N, N, ni) if args.gens == "verifier" else gens
        verify = lambda: P.NIZK.verify_status(ctx, inst, proof, inst.inputs, vgens, LABEL)
        if verify() != 1:
            raise SystemExit("2^%d: the device verifier rejected the prover's proof" % s)
        med, lo, hi = median_ms(verify, WARM, REPS)
        t0 = L.sp_ctx_trips(raw); verify(); trips = L.sp_ctx_trips(raw) - t0
        L.sp_prof_enable(raw, ctypes.c_int(1)); L.sp_prof_reset(raw)
        for _ in range(5):
            verify()
        mv_ms, mv_n = family(raw, "msm_var")
        sp_ms, sp_n = family(raw, "sparse")
        L.sp_prof_enable(raw, ctypes.c_int(0))
        oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
        og = vp(orc.orc_nizk_gens_new(sz(N), sz(N), sz(ni)))
        overify = lambda: orc.orc_nizk_verify_bytes(proof, sz(len(proof)), oi, og, digest, sz(len(digest)), LABEL)
        if overify() != 1:
            raise SystemExit("2^%d: the oracle rejected the prover's proof" % s)
        omed, olo, ohi = median_ms(overify, 0, 3)
        orc.orc_nizk_gens_free(og); orc.orc_instance_free(oi)
        lines += ["synthetic 2^%d: proof %d bytes, C_LZ over %d points, %d round trips per verification" % (s, len(proof), 1 << (s // 2), trips),
                  "  (a) NIZK.verify, device                  median %9.3f ms   (min %.3f, max %.3f)" % (med, lo, hi),
                  "  (b) msm_var launch chain                 mean   %9.3f ms   (of %d); sparse evaluation kernels %.3f ms per verification" % (
                      mv_ms / max(mv_n, 1), mv_n, sp_ms / 5),
                  "  (c) oracle orc_nizk_verify_bytes         median %9.3f ms   (min %.3f, max %.3f)" % (omed, olo, ohi),
                  "  (c) / (a) = %.1f" % (omed / med)]
        if s == 20:
            lines.append("  reference, published for its own machine (BASELINE.md): NIZK::verify 414.5 ms")
        print("\n".join(lines[-6:]), flush=True)
        if vgens is not gens:
            vgens.free()
        gens.free(); inst.free()
    ctx.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
