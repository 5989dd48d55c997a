"""What the device satisfiability check costs (Instance::is_sat -> sp_r1cs_check) next to what a caller had to compose before it existed and to
the oracle's R1CSShape::is_sat on the host cores. One process, its own time limit, stops at the first step that fails. Three instances:
synthetic 2^20, synthetic 2^22 (one entry per row and matrix) and a skewed instance with the nnz of the 2^20 one — three rows of 2^20 - 3
entries, one per matrix, plus 300 rows of 1-3 entries in 2^12 constraints. Per instance:
  (a) Instance.is_sat with a resident VarsAssignment: z built on the device, one fused pass, 16 bytes back;
  (b) the same verdict from entry points the check does not touch: z built the same way, 3 x sp_sparse_mulvec, 3 x sp_table_download, then
      the Montgomery multiplications on one host core (bench/is_sat_host.cc);
  (c) the oracle's is_sat on 16 host threads.
(a) and (b) are medians of 20 calls after 3 warm-ups, timed with the host clock around calls that end in a wait for the device.
usage: python bench/is_sat_probe.py [--out profiles/is_sat.txt]"""
import argparse, ctypes, faulthandler, os, random, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
faulthandler.dump_traceback_later(380, exit=True)   # the probe's own time limit

from spartan_amd import capi, prover as P
from tests.helpers import Q, load_oracle, mont_bulk, sz, vp

WARM, REPS = 3, 20
L = capi.lib


def host_lib():
    so, src = os.path.join(ROOT, "bench", "is_sat_host.so"), os.path.join(ROOT, "bench", "is_sat_host.cc")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", src, "-o", so])
    h = ctypes.CDLL(so)
    h.isat_host_count.restype = sz
    return h


def ok(rc, what):
    if rc != 0:
        raise SystemExit(f"{what} failed: {rc}")


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def skewed(orc, num_cons, num_vars, num_inputs, n_short):
    """entries, canonical values and a satisfying assignment: row k (k = 0, 1, 2) is long in matrix k, over the first num_vars - 3 variables"""
    rng = random.Random(7)
    n = num_vars - 3
    const = num_vars
    v = [rng.getrandbits(248) for _ in range(num_vars)]
    inputs = [rng.getrandbits(248) for _ in range(num_inputs)]
    mats = [[], [], []]
    for k in range(3):
        raw = rng.randbytes(31 * n)
        coef = [int.from_bytes(raw[31 * j:31 * j + 31], "little") for j in range(n)]
        v[n + k] = sum(c * x for c, x in zip(coef, v)) % Q          # the variable the row's other side selects
        mats[k] += [(k, j, coef[j]) for j in range(n)]
    mats[1].append((0, const, 1)); mats[2].append((0, n, 1))          # row 0: (A z) * 1 = v[n]
    mats[0].append((1, const, 1)); mats[2].append((1, n + 1, 1))      # row 1: 1 * (B z) = v[n + 1]
    mats[0].append((2, n + 2, 1)); mats[1].append((2, const, 1))      # row 2: v[n + 2] * 1 = (C z)
    for r in range(3, 3 + n_short):
        ea = [(r, rng.randrange(n), rng.getrandbits(248)) for _ in range(rng.randint(1, 3))]
        eb = [(r, rng.randrange(n), rng.getrandbits(248)) for _ in range(rng.randint(1, 3))]
        a = sum(x * v[c] for _, c, x in ea) % Q
        b = sum(x * v[c] for _, c, x in eb) % Q
        mats[0] += ea; mats[1] += eb; mats[2].append((r, const, a * b % Q))
    ent = mats[0] + mats[1] + mats[2]
    nnz = [len(m) for m in mats]
    rows = (ctypes.c_uint64 * len(ent))(*[e[0] for e in ent]); cols = (ctypes.c_uint64 * len(ent))(*[e[1] for e in ent])
    vals = b"".join(e[2].to_bytes(32, "little") for e in ent)
    return nnz, rows, cols, vals, mont_bulk(v), mont_bulk(inputs)


def measure(name, ctx, orc, host, inst, oi, ncons, num_vars, num_inputs, vars_, inputs, out):
    """num_vars is a power of two above num_inputs + 1 here, ncons a power of two: Instance::new pads neither"""
    raw = ctx.raw()

    class Raw:   # spartan_amd.capi's helpers take an object with the sp_ctx* in .h
        h = raw
    nnz = [orc.orc_instance_nnz(oi, ctypes.c_int(k)) for k in range(3)]
    tot = sum(nnz)
    rows = (ctypes.c_uint64 * tot)(); cols = (ctypes.c_uint64 * tot)(); vals = (ctypes.c_uint64 * (4 * tot))()
    ov = (ctypes.c_uint64 * (4 * num_vars))(); oin = (ctypes.c_uint64 * (4 * max(num_inputs, 1)))()
    orc.orc_instance_export(oi, rows, cols, vals, ov, oin)
    nvp = num_vars
    # (a)
    va = P.VarsAssignment(ctx, vars_)
    if inst.is_sat(va, inputs) is not True:
        raise SystemExit(name + ": the device check rejects a satisfying assignment")
    a = timed(lambda: inst.is_sat(va, inputs))
    # (b): the caller's own matrix handles, its resident assignment, and per call z, three products, three downloads, the host loop
    hs, off = [], 0
    for k in range(3):
        h = vp()
        ok(L.sp_sparse_upload(raw, ctypes.byref(rows, 8 * off), ctypes.byref(cols, 8 * off), ctypes.byref(vals, 32 * off), sz(nnz[k]), sz(ncons), sz(2 * nvp),
                              ctypes.byref(h)), "sp_sparse_upload")
        hs.append(h); off += nnz[k]
    res = capi.Table.upload(Raw, vars_, num_vars)
    tail = (ctypes.c_uint64 * (4 * (1 + num_inputs)))()
    R = 2**256 % Q
    for w in range(4):
        tail[w] = (R >> (64 * w)) & (2**64 - 1)
    for w in range(4 * num_inputs):
        tail[4 + w] = inputs[w]
    bufs = [(ctypes.c_uint64 * (4 * ncons))() for _ in range(3)]
    parts = {"device": 0.0, "host": 0.0}

    def composed():
        t0 = time.perf_counter()
        z = vp()
        ok(L.sp_table_alloc(raw, sz(2 * nvp), ctypes.byref(z)), "sp_table_alloc")
        ok(L.sp_table_copy(raw, z, sz(0), res.h, sz(0), sz(num_vars)), "sp_table_copy")
        ok(L.sp_table_write(raw, z, sz(nvp), tail, sz(1 + num_inputs)), "sp_table_write")
        ts = []
        for h in hs:
            t = vp()
            ok(L.sp_sparse_mulvec(raw, h, z, ctypes.byref(t)), "sp_sparse_mulvec")
            ts.append(t)
        for t, b in zip(ts, bufs):
            ok(L.sp_table_download(raw, t, sz(0), sz(ncons), b), "sp_table_download")
        t1 = time.perf_counter()
        bad = host.isat_host_count(bufs[0], bufs[1], bufs[2], sz(ncons))
        t2 = time.perf_counter()
        for t in ts + [z]:
            L.sp_table_free(t)
        parts["device"] += t1 - t0; parts["host"] += t2 - t1
        if bad != 0:
            raise SystemExit(name + ": the composed check rejects a satisfying assignment")
    b = timed(composed)
    n = WARM + REPS
    # (c)
    orc.orc_set_threads(ctypes.c_int(16))
    cs = []
    for _ in range(3):
        t0 = time.perf_counter()
        if orc.orc_instance_is_sat(oi) != 1:
            raise SystemExit(name + ": the oracle rejects the assignment")
        cs.append((time.perf_counter() - t0) * 1e3)
    cs.sort()
    alg = sum(nnz) * 68 + 12 * (ncons + 1)
    out.append(f"{name}: constraints {ncons}, columns {2 * nvp}, nnz {nnz[0]} + {nnz[1]} + {nnz[2]}, algorithmic bytes {alg / 1e6:.1f} MB")
    out.append(f"  (a) Instance.is_sat, resident assignment     median {a[0]:9.3f} ms   (min {a[1]:.3f}, max {a[2]:.3f})   {alg / a[0] / 1e6:.1f} GB/s algorithmic")
    out.append(f"  (b) 3 mulvec + 3 downloads + host loop       median {b[0]:9.3f} ms   (min {b[1]:.3f}, max {b[2]:.3f})   mean split: device + PCIe {parts['device'] / n * 1e3:.3f} ms, host loop {parts['host'] / n * 1e3:.3f} ms")
    out.append(f"  (c) oracle is_sat, 16 host threads           median {cs[1]:9.3f} ms   (of 3)")
    out.append(f"  (b) / (a) = {b[0] / a[0]:.1f}   (c) / (a) = {cs[1] / a[0]:.1f}")
    for h in hs:
        L.sp_sparse_free(h)
    res.free(); va.free()
    return a[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "is_sat.txt"))
    args = ap.parse_args()
    orc, host = load_oracle(), host_lib()
    ctx = P.Ctx(0)
    out = ["Instance::is_sat on the device against the composed check and the oracle (bench/is_sat_probe.py; medians of %d calls after %d warm-ups)" % (REPS, WARM), ""]
    med = {}
    for s in (20, 22):
        N = 1 << s
        orc.orc_set_threads(ctypes.c_int(16))
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=s)
        oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(10), ctypes.c_uint64(s)))
        med[s] = measure("synthetic 2^%d" % s, ctx, orc, host, inst, oi, N, N, 10, inst.vars, inst.inputs, out)
        orc.orc_instance_free(oi); inst.free()
        print("\n".join(out[-5:]), flush=True)
    num_cons, num_vars, ni = 1 << 12, 1 << 20, 2
    nnz, rows, cols, vals, bv, bi = skewed(orc, num_cons, num_vars, ni, 300)
    inst = P.Instance.new(ctx, num_cons, num_vars, ni, nnz, rows, cols, vals)
    err = ctypes.c_int(0)
    oi = vp(orc.orc_instance_new_padded(sz(num_cons), sz(num_vars), sz(ni), (sz * 3)(*nnz), rows, cols, vals, bv, sz(num_vars), bi, ctypes.byref(err)))
    if err.value != 0 or not oi:
        raise SystemExit("the oracle refuses the skewed instance")
    med["skew"] = measure("skewed, nnz of 2^20", ctx, orc, host, inst, oi, num_cons, num_vars, ni, bv, bi, out)
    orc.orc_instance_free(oi); inst.free()
    out.append("")
    out.append("(a) skewed / (a) synthetic 2^20 = %.2f at nearly equal nnz" % (med["skew"] / med[20]))
    print("\n".join(out[-7:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    ctx.close()
    faulthandler.cancel_dump_traceback_later()


if __name__ == "__main__":
    main()
