"""What Instance::new costs, one entry list three ways: Instance.new (the host path: a loop over every entry that checks, converts and copies
it, two more host copies, two counting sorts and ten pageable uploads per matrix), Instance.from_entries (the same host arrays; indices and
bytes uploaded, everything else on the device: sp_sparse_from_entries) and Instance.from_tensors (the arrays already on the GPU:
sp_sparse_from_entries_dev). 2^log2 constraints and variables, ten inputs, about three entries per row and matrix, generated here. One
process, its own time limit. The three are timed ALTERNATELY, 20 rounds after 3 warm-up rounds, host clock around the constructor alone (it
ends in a wait for the device; the instance is freed outside the timed span); median, minimum and maximum of each.
usage: python bench/instance_probe.py [--log2 16 20] [--out profiles/instance_from_entries.txt]"""
import argparse, ctypes, faulthandler, os, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
faulthandler.dump_traceback_later(540, exit=True)   # the probe's own time limit

import numpy as np
import torch
from spartan_amd import prover as P

WARM, REPS = 3, 20
sz = ctypes.c_size_t


def entry_list(rng, nc, nv, ni, per_row=3):
    """one matrix: per_row entries in every row, in shuffled order; columns over the variables, the constant and the inputs; values below 2^252"""
    n = per_row * nc
    rows = np.repeat(np.arange(nc, dtype=np.uint64), per_row)
    rng.shuffle(rows)
    cols = rng.integers(0, nv + 1 + ni, size=n, dtype=np.uint64)
    vals = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    vals[:, 31] &= 0x0f
    return rows, cols, vals.reshape(-1)


def shape_bincode(inst):
    H = P.H
    n = H.spz_instance_shape_bincode(inst.h, None, sz(0))
    buf = (ctypes.c_uint8 * n)()
    H.spz_instance_shape_bincode(inst.h, buf, sz(n))
    return bytes(buf)


def run(ctx, log2):
    nc = nv = 1 << log2
    ni = 10
    rng = np.random.default_rng(log2)
    mats = [entry_list(rng, nc, nv, ni) for _ in range(3)]
    nnz = [len(m[0]) for m in mats]
    total = sum(nnz)
    rows = np.ascontiguousarray(np.concatenate([m[0] for m in mats])); cols = np.ascontiguousarray(np.concatenate([m[1] for m in mats]))
    vals = np.ascontiguousarray(np.concatenate([m[2] for m in mats]))
    crows = (ctypes.c_uint64 * total).from_buffer(rows); ccols = (ctypes.c_uint64 * total).from_buffer(cols)
    cvals = (ctypes.c_uint8 * (32 * total)).from_buffer(vals)
    dev = [(torch.from_numpy(m[0].view(np.int64)).cuda(), torch.from_numpy(m[1].view(np.int64)).cuda(), torch.from_numpy(m[2]).cuda()) for m in mats]
    torch.cuda.synchronize()

    legs = [("Instance.new (host loop, sorts, pageable uploads)", lambda: P.Instance.new(ctx, nc, nv, ni, nnz, crows, ccols, cvals)),
            ("Instance.from_entries (upload + device build)", lambda: P.Instance.from_entries(ctx, nc, nv, ni, nnz, crows, ccols, cvals)),
            ("Instance.from_tensors (device build, no upload)", lambda: P.Instance.from_tensors(ctx, nc, nv, ni, *dev))]
    if log2 <= 16:   # same instance first: the serialised shape (every stored entry, in order) is the same three ways
        made = [fn() for _, fn in legs]
        ref = shape_bincode(made[0])
        assert all(shape_bincode(i) == ref for i in made[1:])
        for i in made:
            i.free()
    ts = {name: [] for name, _ in legs}
    for r in range(WARM + REPS):
        for name, fn in legs:
            t0 = time.perf_counter()
            inst = fn()
            dt = (time.perf_counter() - t0) * 1e3
            inst.free()
            if r >= WARM:
                ts[name].append(dt)
    lines = ["# 2^%d constraints, 2^%d variables, %d inputs; %d entries per matrix (%d in all: %.1f MB of indices and value bytes); %d alternating "
             "rounds after %d warm-ups; ms" % (log2, log2, ni, nnz[0], total, 48 * total / 1e6, REPS, WARM),
             "%-52s %10s %10s %10s" % ("leg", "median", "min", "max")]
    med = {}
    for name, _ in legs:
        t = sorted(ts[name])
        med[name] = t[len(t) // 2]
        lines.append("%-52s %10.3f %10.3f %10.3f" % (name, med[name], t[0], t[-1]))
    base = med[legs[0][0]]
    lines.append("Instance.new / from_entries: %.2fx; Instance.new / from_tensors: %.2fx (medians)" % (base / med[legs[1][0]], base / med[legs[2][0]]))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = P.Ctx(0)
    lines = ["# python bench/instance_probe.py --log2 %s" % " ".join(str(x) for x in a.log2)]
    for log2 in a.log2:
        lines += run(ctx, log2) + [""]
    text = "\n".join(lines)
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)
    ctx.close()


if __name__ == "__main__":
    main()
