"""What NIZK::verify costs on the device (spartan_amd/host/verifier.cc) next to the oracle's restated verifier on the host cores of the same
box. One process, its own time limit, stops at the first step that fails. Per size (2^16, 2^20, 2^22 constraints, synthetic instances):
  (a) NIZK.verify of the HIP prover's proof, warm (digest set, generator tables built, one verification done): median of 20 calls timed with
      the host clock — the call ends in a wait for the device, so the wall time is the verification;
  (b) the msm_var kernel chain of one verification (sp_prof_*, HIP events; collected in runs of their own, not in the timed ones) and the
      round trips of one verification (sp_ctx_trips);
  (c) the oracle's orc_nizk_verify_bytes on the same bytes, 16 host threads, median of 3.
The reference publishes 414.5 ms for NIZK::verify at 2^20 on its own machine: context, not a comparison on this box.
usage: python bench/verify_probe.py [--out profiles/nizk_verify.txt] [--sizes 16,20,22]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="16,20,22")
    args = ap.parse_args()
    orc = load_oracle()
    orc.orc_set_threads(ctypes.c_int(16))
    lines = ["NIZK::verify on the device against the oracle's verifier on the host (bench/verify_probe.py; host CPU: %s)" % cpu_model(),
             "(a): median of %d warm calls, host clock; msm_var: HIP events around its launch chain, runs of their own; (c): median of 3, 16 threads" % REPS,
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
        verify = lambda: P.NIZK.verify_status(ctx, inst, proof, inst.inputs, gens, LABEL)
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
        gens.free(); inst.free()
    ctx.close()
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
