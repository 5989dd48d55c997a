"""What it costs to hand the prover a witness as canonical bytes (VarsAssignment.from_bytes -> sp_table_from_bytes: upload + one in-place pass
on the device) next to the upload of ready Montgomery limbs (VarsAssignment(ctx, limbs): the same 32 n bytes over PCIe, no pass) and next to
the conversion a caller would otherwise run on one host core (spz_scalars_from_bytes). One process, its own time limit. The three are timed
ALTERNATELY, 20 rounds after 3 warm-up rounds, host clock around calls that end in a wait for the device; median, minimum and maximum of each.
usage: python bench/assignment_bytes_probe.py [--log2 20] [--out profiles/assignment_bytes.txt]"""
import argparse, ctypes, faulthandler, os, random, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
faulthandler.dump_traceback_later(300, exit=True)   # the probe's own time limit

from spartan_amd import prover as P
from tests.helpers import Q, R

WARM, REPS = 3, 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = 1 << a.log2
    rng = random.Random(20)
    vals = [rng.getrandbits(300) % Q for _ in range(n)]
    data = b"".join(v.to_bytes(32, "little") for v in vals)
    limbs = (ctypes.c_uint64 * (4 * n)).from_buffer_copy(b"".join((v * R % Q).to_bytes(32, "little") for v in vals))
    host_out = (ctypes.c_uint64 * (4 * n))()
    rep = (ctypes.c_uint64 * 2)()
    ctx = P.Ctx(0)

    def from_bytes():
        P.VarsAssignment.from_bytes(ctx, data).free()

    def from_limbs():
        P.VarsAssignment(ctx, limbs).free()

    def host_parse():
        assert P.H.spz_scalars_from_bytes(data, ctypes.c_size_t(n), host_out, rep) == 0

    # same results first: the device parse and the host parse both give the limbs the plain upload is handed
    va = P.VarsAssignment.from_bytes(ctx, data)
    assert va.to_bytes() == data and va.check_reduced() == (0, None)
    va.free()
    host_parse()
    assert bytes(host_out) == bytes(limbs)

    legs = [("VarsAssignment.from_bytes (upload + device pass)", from_bytes), ("VarsAssignment(ctx, limbs) (upload only)", from_limbs),
            ("spz_scalars_from_bytes (one host core, no upload)", host_parse)]
    ts = {name: [] for name, _ in legs}
    for r in range(WARM + REPS):
        for name, fn in legs:
            t0 = time.perf_counter()
            fn()
            if r >= WARM:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    lines = ["# python bench/assignment_bytes_probe.py --log2 %d   (n = 2^%d scalars, %d MB; %d alternating rounds after %d warm-ups; ms)" % (a.log2, a.log2, 32 * n >> 20, REPS, WARM),
             "%-52s %9s %9s %9s" % ("leg", "median", "min", "max")]
    for name, _ in legs:
        t = sorted(ts[name])
        lines.append("%-52s %9.3f %9.3f %9.3f" % (name, t[len(t) // 2], t[0], t[-1]))
    fb, fl = sorted(ts[legs[0][0]]), sorted(ts[legs[1][0]])
    lines.append("from_bytes - upload, medians: %+.3f ms; spread of the upload's %d samples (max - min): %.3f ms" % (fb[REPS // 2] - fl[REPS // 2], REPS, fl[-1] - fl[0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
