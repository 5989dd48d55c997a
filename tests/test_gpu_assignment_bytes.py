"""Canonical scalar bytes -> resident assignments on the device (spartan_amd/csrc/assign.hip: sp_table_from_bytes, sp_table_from_bytes_dev,
sp_table_to_bytes, sp_table_check_reduced) and everything above them (VarsAssignment.from_bytes / from_tensor / to_bytes / check_reduced,
InputsAssignment.from_bytes, InvalidScalar). Everything is compared EXACTLY with the Python-integer model of tests/assign_reference.py:
the Montgomery limbs, the bytes that come back, the count of refused entries and the lowest refused index wherever it sits in a wavefront
or a workgroup. The end-to-end tests prove from a bytes-made assignment and want the proof of the limbs-made one and of the oracle."""
import ctypes, os, re, struct
import pytest
from tests.helpers import *
from tests import assign_reference as ar
from tests import structured_cases as sc

pytestmark = pytest.mark.gpu
SP_EINVAL, SP_ESCALAR = -1, -5
u8p = ctypes.POINTER(ctypes.c_uint8)


def _block_size():
    src = open(os.path.join(ROOT, "spartan_amd", "csrc", "assign.hip")).read()
    m = re.search(r"constexpr unsigned ASSIGN_BLOCK = (\d+);", src)
    assert m and src.count("(n + ASSIGN_BLOCK - 1) / ASSIGN_BLOCK") == 1 and "gridDim" not in src   # one lane per scalar: no cap, no stride
    return int(m.group(1))


B = _block_size()
SIZES = sorted({1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 4099, 65537})


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def L():
    from spartan_amd import capi
    return capi.lib


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


def _pack(limbs):
    return struct.pack("<%dQ" % len(limbs), *limbs)


def _from_bytes(L, ctx, data, n, dev=False):
    """(rc, table handle, (count, first)); data: bytes (host) or a device address"""
    h = vp(0xdead)
    rep = (ctypes.c_uint64 * 2)(7, 7)
    f = L.sp_table_from_bytes_dev if dev else L.sp_table_from_bytes
    rc = f(ctx.raw(), vp(data) if dev else data, sz(n), ctypes.byref(h), rep)
    return rc, h, (int(rep[0]), int(rep[1]))


def _download(L, ctx, h, n):
    out = (ctypes.c_uint64 * (4 * n))()
    assert L.sp_table_download(ctx.raw(), h, sz(0), sz(n), out) == 0
    return bytes(out)


def _to_bytes(L, ctx, h, off, n):
    out = (ctypes.c_uint8 * (32 * n))()
    assert L.sp_table_to_bytes(ctx.raw(), h, sz(off), sz(n), out) == 0
    return bytes(out)


def _check_reduced(L, ctx, h, off, n):
    rep = (ctypes.c_uint64 * 2)(7, 7)
    assert L.sp_table_check_reduced(ctx.raw(), h, sz(off), sz(n), rep) == 0
    return int(rep[0]), int(rep[1])


def _valid_conversion_is_correct(L, ctx, n=257, seed=99):
    data = ar.enc(ar.valid_values(n, seed))
    rc, h, rep = _from_bytes(L, ctx, data, n)
    assert rc == 0 and rep == (0, ar.NONE)
    assert _download(L, ctx, h, n) == _pack(ar.from_bytes(data)[0])
    L.sp_table_free(h)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_limbs_bytes_and_check_match_the_model(L, ctx, n):
    data = ar.enc(ar.valid_values(n, n))
    want, count, first = ar.from_bytes(data)
    rc, h, rep = _from_bytes(L, ctx, data, n)
    assert rc == 0 and rep == (0, ar.NONE) == (count, first)
    assert L.sp_table_len(h) == n
    assert _download(L, ctx, h, n) == _pack(want)
    assert _to_bytes(L, ctx, h, 0, n) == data
    assert _check_reduced(L, ctx, h, 0, n) == (0, ar.NONE)
    if n > 65:                                            # a sub-range that starts and ends inside wavefronts
        assert _to_bytes(L, ctx, h, 3, n - 5) == data[32 * 3:32 * (n - 2)]
    L.sp_table_free(h)


def _refused(L, ctx, vals, positions, bad_values):
    bad = list(vals)
    for k, p in enumerate(positions):
        bad[p] = bad_values[k % len(bad_values)]
    data = ar.enc(bad)
    rc, h, rep = _from_bytes(L, ctx, data, len(bad))
    assert rc == SP_ESCALAR and not h.value, (positions, rc)
    assert rep == (len(positions), min(positions)) == ar.from_bytes(data)[1:], positions


@pytest.mark.parametrize("k", range(len(ar.EDGE_INVALID)))
def test_one_invalid_entry_is_refused_wherever_it_sits(L, ctx, k):
    vals = ar.valid_values(257, 5)
    for pos in (0, 63, 64, 65, 128, 255, 256):
        _refused(L, ctx, vals, [pos], [ar.EDGE_INVALID[k]])
    _valid_conversion_is_correct(L, ctx)


def test_several_invalid_entries_count_and_lowest_index(L, ctx):
    vals = ar.valid_values(257, 6)
    for positions in ([70, 200], [200, 70], [3, 130, 256], [256, 130, 3],       # different wavefronts, either order of values
                      [66, 67], [127, 64], [192, 193, 255], [10, 11, 12],       # one wavefront
                      [63, 64], [255, 256], [0, 256]):                          # across a wavefront and a workgroup boundary
        _refused(L, ctx, vals, positions, ar.EDGE_INVALID)
    _valid_conversion_is_correct(L, ctx)
    _refused(L, ctx, vals, list(range(257)), ar.EDGE_INVALID)                   # all of them: (257, 0)
    _valid_conversion_is_correct(L, ctx)


@pytest.mark.parametrize("n", [65, 4099])
def test_device_source_through_from_tensor(P, ctx, n):
    import torch                                          # the first case pays for the process's import of torch and its device set-up
    vals = ar.valid_values(n, 1000 + n)
    data = ar.enc(vals)
    t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    big = torch.empty(32 * n + 9, dtype=torch.uint8, device="cuda")   # (empty, and copies below: no torch kernel is loaded for this test)
    view = big[1:1 + 32 * n]                              # starts one byte into a larger tensor
    view.copy_(t)
    assert view.data_ptr() % 2 == 1
    for src in (t, view):
        torch.cuda.synchronize()
        a = P.VarsAssignment.from_tensor(ctx, src)
        assert a.n == n and a.to_bytes() == data and a.check_reduced() == (0, None)
        a.free()
    for positions in ([0], [n - 1], [n // 2, 64], [n - 1, 63, 1]):
        assert len(set(positions)) == len(positions)
        bad = list(vals)
        for k, p in enumerate(positions):
            bad[p] = ar.EDGE_INVALID[(k + n) % len(ar.EDGE_INVALID)]
        view.copy_(torch.frombuffer(bytearray(ar.enc(bad)), dtype=torch.uint8).cuda())
        torch.cuda.synchronize()
        with pytest.raises(P.InvalidScalar) as e:
            P.VarsAssignment.from_tensor(ctx, view)
        assert (e.value.count, e.value.first) == (len(positions), min(positions))
        assert "InvalidScalar: entry %d (%d of %d entries are not canonical)" % (min(positions), len(positions), n) in str(e.value)
    view.copy_(t)
    torch.cuda.synchronize()
    a = P.VarsAssignment.from_tensor(ctx, view)           # the context after the refusals
    assert a.to_bytes() == data
    a.free()
    with pytest.raises(P.SpartanHipError):
        P.VarsAssignment.from_tensor(ctx, big[:33])
    with pytest.raises(P.SpartanHipError):
        P.VarsAssignment.from_tensor(ctx, big[:64:2])


def test_unreduced_limbs_are_found_by_check_reduced(L, ctx):
    raw = [x for v in (Q - 1, Q, 2**256 - 1, 0) for x in ar._limbs(v)]
    h = vp()
    assert L.sp_table_upload(ctx.raw(), (ctypes.c_uint64 * 16)(*raw), sz(4), ctypes.byref(h)) == 0
    assert _check_reduced(L, ctx, h, 0, 4) == (2, 1) == ar.check_reduced(raw)
    for off, n in ((0, 1), (1, 1), (2, 2), (3, 1), (1, 3), (2, 1)):
        assert _check_reduced(L, ctx, h, off, n) == ar.check_reduced(raw, off, n), (off, n)
    assert _check_reduced(L, ctx, h, 2, 2) == (1, 2)     # its own first index, counted from the start of the table
    assert _download(L, ctx, h, 4) == _pack(raw)         # the check changes nothing
    L.sp_table_free(h)


def test_argument_checks_write_nothing(L, ctx):
    rc, h, rep = _from_bytes(L, ctx, None, 4)
    assert rc == SP_EINVAL and h.value == 0xdead and rep == (7, 7)
    rc, h, rep = _from_bytes(L, ctx, bytes(64), 0)
    assert rc == SP_EINVAL and h.value == 0xdead and rep == (7, 7)
    rc, h, rep = _from_bytes(L, ctx, 0, 4, dev=True)
    assert rc == SP_EINVAL and h.value == 0xdead and rep == (7, 7)
    data = ar.enc(ar.valid_values(8, 1))
    rc, t, _ = _from_bytes(L, ctx, data, 8)
    assert rc == 0
    out = (ctypes.c_uint8 * (32 * 16))(*([9] * 512))
    rep = (ctypes.c_uint64 * 2)(7, 7)
    for off, n in ((0, 9), (8, 1), (5, 4), (0, 0), (2**64 - 1, 2), (1, 2**64 - 1)):
        assert L.sp_table_to_bytes(ctx.raw(), t, sz(off), sz(n), out) == SP_EINVAL, (off, n)
        assert L.sp_table_check_reduced(ctx.raw(), t, sz(off), sz(n), rep) == SP_EINVAL, (off, n)
    assert L.sp_table_to_bytes(ctx.raw(), t, sz(0), sz(8), None) == SP_EINVAL
    assert bytes(out) == bytes([9] * 512) and list(rep) == [7, 7]
    assert L.sp_table_check_reduced(ctx.raw(), t, sz(0), sz(8), None) == 0      # report may be NULL
    assert _to_bytes(L, ctx, t, 7, 1) == data[32 * 7:]
    L.sp_table_free(t)


def test_python_buffers_and_errors(P, ctx):
    import numpy as np
    vals = ar.valid_values(100, 2)
    data = ar.enc(vals)
    for buf in (data, bytearray(data), memoryview(data), np.frombuffer(data, dtype=np.uint8).copy(), np.frombuffer(data, dtype=np.uint8)):
        a = P.VarsAssignment.from_bytes(ctx, buf)
        assert a.n == 100 and a.to_bytes() == data and a.check_reduced() == (0, None)
        a.free()
    with pytest.raises(P.SpartanHipError):
        P.VarsAssignment.from_bytes(ctx, data[:-1])
    limbs = P.VarsAssignment(ctx, mont_bulk(vals))       # the constructor from Montgomery limbs holds the same table
    assert limbs.to_bytes() == data
    limbs.free()


def _proofs(P, ctx, inst, gens, ngens, enc, vars_, inputs, tape):
    return (P.SNARK.prove(ctx, inst, enc, vars_, inputs, gens, sc.SNARK_LABEL, tape), P.NIZK.prove(ctx, inst, vars_, inputs, ngens, sc.NIZK_LABEL, tape))


def _end_to_end(P, ctx, inst, gens, ngens, enc, nvars, limbs, inputs_limbs, ninputs, tape, want_snark, want_nizk, breaking_var):
    """limbs -> canonical bytes (tests.helpers.from_mont_bulk) -> assignments made from bytes: same satisfiability, same proofs, both verify"""
    vals = from_mont_bulk(limbs, nvars)
    data = ar.enc(vals)
    in_data = ar.enc(from_mont_bulk(inputs_limbs, ninputs))
    va = P.VarsAssignment.from_bytes(ctx, data)
    inputs = P.InputsAssignment.from_bytes(in_data)
    assert va.n == nvars and bytes(inputs) == bytes(inputs_limbs)[:32 * ninputs]
    assert inst.is_sat(va, inputs) is True
    snark, nizk = _proofs(P, ctx, inst, gens, ngens, enc, va, inputs, tape)
    snark_l, nizk_l = _proofs(P, ctx, inst, gens, ngens, enc, limbs, inputs_limbs, tape)
    assert snark == snark_l == want_snark
    assert nizk == nizk_l == want_nizk
    comm = enc.commitment(ctx)
    assert P.SNARK.verify_status(ctx, comm, snark, inputs, gens, sc.SNARK_LABEL) == 1
    assert P.NIZK.verify_status(ctx, inst, nizk, inputs, ngens, sc.NIZK_LABEL) == 1
    comm.free()
    # one byte of one variable changed to another canonical value: a violated constraint; to q's bytes: refused at that index
    j = breaking_var
    other = bytearray(data); other[32 * j] ^= 1
    assert int.from_bytes(other[32 * j:32 * j + 32], "little") < Q
    vb = P.VarsAssignment.from_bytes(ctx, other)
    rep = inst.check(vb, inputs)
    assert rep.violated >= 1 and rep.first_row is not None
    vb.free()
    refused = bytearray(data); refused[32 * j:32 * j + 32] = Q.to_bytes(32, "little")
    with pytest.raises(P.InvalidScalar) as e:
        P.VarsAssignment.from_bytes(ctx, refused)
    assert (e.value.first, e.value.count) == (j, 1)
    assert inst.is_sat(va, inputs) is True               # the context and the assignment after the refusal
    va.free()


def test_end_to_end_synthetic_byte_parity(P, ctx, orc):
    N, ni, seed = 1024, 10, 41
    inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, ni, seed=seed)
    inst.set_digest(b"assignment-bytes")
    gens = P.SNARKGens(ctx, N, N, ni, N); ngens = P.NIZKGens(ctx, N, N, ni)
    enc = P.SNARK.encode(ctx, inst, gens)
    tape = P.seed_scalar(b"tape", seed)
    orc.orc_set_threads(ctypes.c_int(16))
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    og = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(ni), sz(N)))
    oe = vp(orc.orc_snark_encode(oi, og))
    op = vp(orc.orc_snark_prove(oi, og, oe, sc.SNARK_LABEL, tape, None))
    ong = vp(orc.orc_nizk_gens_new(sz(N), sz(N), sz(ni)))
    onp = vp(orc.orc_nizk_prove(oi, ong, b"assignment-bytes", sz(16), sc.NIZK_LABEL, tape, None))
    want_snark, want_nizk = sc.oracle_bytes(orc, orc.orc_proof_bytes, op), sc.oracle_bytes(orc, orc.orc_proof_bytes, onp)
    # the synthetic instance's row i reads variable i: changing any variable breaks a row
    _end_to_end(P, ctx, inst, gens, ngens, enc, N, inst.vars, inst.inputs, ni, tape, want_snark, want_nizk, breaking_var=N - 1)
    orc.orc_proof_free(op); orc.orc_proof_free(onp); orc.orc_encode_free(oe)
    orc.orc_snark_gens_free(og); orc.orc_nizk_gens_free(ong); orc.orc_instance_free(oi)
    enc.free(); ngens.free(); gens.free(); inst.free()


def test_end_to_end_shifted_byte_parity(P, ctx, orc):
    """37 constraints, 100 variables, 7 inputs: the assignment is shorter than the padded num_vars (128), so prove pads a bytes-made table"""
    name = "shifted"
    orc.orc_set_threads(ctypes.c_int(1))
    run = sc.oracle_run(orc, name)
    pk = run.pk
    inst = P.Instance.new(ctx, pk.num_cons, pk.num_vars, pk.num_inputs, pk.nnz, pk.rows, pk.cols, pk.vals)
    inst.set_digest(run.digest)
    gens = P.SNARKGens(ctx, *run.gens_args); ngens = P.NIZKGens(ctx, *run.gens_args[:3])
    enc = P.SNARK.encode(ctx, inst, gens)
    tape = P.seed_scalar(b"tape", sc.TAPE_SEED[name])
    assert ar.enc(run.case[6]) == ar.enc(from_mont_bulk(pk.vars, pk.num_vars))   # the canonical bytes ARE the case's integers
    _end_to_end(P, ctx, inst, gens, ngens, enc, pk.num_vars, pk.vars, pk.inputs, pk.num_inputs, tape, run.snark, run.nizk,
                breaking_var=sc.BREAKING_VAR[name])
    enc.free(); ngens.free(); gens.free(); inst.free()
