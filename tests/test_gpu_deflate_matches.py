"""The device's share of R1CSShape::get_digest (spartan_amd/csrc/deflate_match.hip; driven by spartan_amd/host/digest.cc): tdefl's match search
with one input position per lane gives the tables of the host search (spz_deflate_matches_host) element by element, the device-assisted
deflate gives the sequential deflater's bytes, sp_sparse_bincode gives the host serialisation's bytes, and an instance's digest — and so a
NIZK proof — is the same whichever of the two paths computed it. The corpus is that of tests/test_deflate_matches.py; the segment length
(option digest.segment) is set so that the inputs cross several seams, and to 32768 and 65536, where a seam falls on the two moduli of the
search (the dictionary size and the 16-bit chain positions)."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import deflate_corpus as dc

pytestmark = pytest.mark.gpu
SEGMENTS = [49999, 32768, 65536]     # 200000 bytes: four seams at no round position, six at multiples of 32768, three at multiples of 65536


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def corpus(orc):
    return dc.build(orc)


_HOST = {}


def _host(P, corpus, probes):
    """{name: (L, A, B, stream)} of the host search and the sequential deflater at this probe count, computed once"""
    if probes not in _HOST:
        _HOST[probes] = {name: dc.host_tables(P.H, c, probes, links=True) + (dc.zlib_probes(P.H, c, probes),) for name, c in corpus.items()}
    return _HOST[probes]


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_tables_equal_the_host_tables(P, ctx, corpus, probes):
    from spartan_amd.capi import lib
    want = _host(P, corpus, probes)
    for seg in SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, c in corpus.items():
            if seg != SEGMENTS[0] and len(c) <= 32768:
                continue   # one segment whatever the option says: run once
            n = len(c)
            L = (ctypes.c_uint16 * max(1, n))(); A = (ctypes.c_uint32 * max(1, n))(); B = (ctypes.c_uint32 * max(1, n))()
            rc = lib.sp_deflate_matches(ctx.raw(), dc.u8(c), sz(n), ctypes.c_int(0), ctypes.c_uint32(probes), L, A, B)
            assert rc == 0, (name, seg, rc)
            hL, hA, hB, _ = want[name]
            for what, got, ref in (("L", L, hL), ("A", A, hA), ("B", B, hB)):
                p = dc.first_difference(got, ref, n)
                assert p is None, "%s of %s, segment %d, %d probes: first difference at position %d: device %#x, host %#x" % (
                    what, name, seg, probes, p, got[p], ref[p])


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_assisted_stream_equals_the_deflaters(P, ctx, corpus, probes):
    want = _host(P, corpus, probes)
    lookups = fallbacks = 0
    for seg in SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, c in corpus.items():
            if seg != SEGMENTS[0] and len(c) <= 32768:
                continue
            z, st = P.zlib_device(ctx, c, probes)
            assert z == want[name][3], (name, seg, probes)
            assert st["device"] == 1 and st["segments"] == (len(c) + seg - 1) // seg, (name, seg, st)
            lookups += st["lookups"]; fallbacks += st["fallbacks"]
    assert fallbacks * 100 < lookups
    z, _ = P.zlib_device(ctx, corpus["shape/2^9"], 128, old_header=True)
    assert z == dc.zlib_probes(P.H, corpus["shape/2^9"], 128, 1) and z[:2] == b"\x78\x01"


def _random_entries(rng, n, ncols):
    return [(i, rng.randrange(ncols), rng.randrange(Q)) for i in range(n)]


def _pack(A, B, C):
    ent = list(A) + list(B) + list(C)
    u64 = ctypes.c_uint64
    return ([len(A), len(B), len(C)], (u64 * len(ent))(*[e[0] for e in ent]), (u64 * len(ent))(*[e[1] for e in ent]),
            b"".join(e[2].to_bytes(32, "little") for e in ent))


def _host_bincode(P, inst):
    n = P.H.spz_instance_shape_bincode(inst.h, None, sz(0))
    b = (ctypes.c_uint8 * n)()
    P.H.spz_instance_shape_bincode(inst.h, b, sz(n))
    return bytes(b)


def test_device_bincode_equals_the_host_serialisation(P, ctx, orc):
    for s in (4, 9, 12):
        N = 1 << s
        inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=3)      # Instance::new's constructor over host entries
        got = inst.shape_bincode_device()
        assert got == _host_bincode(P, inst), s
        oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(10), ctypes.c_uint64(3)))
        assert got == oracle_shape_bincode(orc, oi), s
        orc.orc_instance_free(oi)
        inst.free()
    rng = random.Random(5)
    N = 1 << 9
    mats = [_random_entries(rng, N - 3 * k, N + 1 + 10) for k in range(3)]     # three different entry counts, columns on both sides of the shift
    new = P.Instance.new(ctx, N, N, 10, *_pack(*mats))
    nnz, rows, cols, vals = _pack(*mats)
    resident = P.Instance.from_entries(ctx, N, N, 10, nnz, rows, cols, bytearray(vals))
    want = _host_bincode(P, new)
    assert len(want) == 24 + 3 * 24 + 48 * sum(nnz)
    assert new.shape_bincode_device() == want and resident.shape_bincode_device() == want and _host_bincode(P, resident) == want
    new.free(); resident.free()


@pytest.mark.parametrize("s", [9, 12])
def test_digest_is_the_same_on_both_paths(P, ctx, s):
    N = 1 << s
    ctx.set_option("digest.segment", 49999)     # 2^9: two segments, 2^12: twelve
    made = {}
    try:
        for old_header in (False, True):
            for device in (0, 1):
                ctx.set_option("digest.device", device)
                inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=3)
                inst.set_digest_header(old_header)
                d = inst.digest()
                st = inst.digest_stats()
                assert st["device"] == device and (st["lookups"] > 0) == bool(device), (device, st)
                made[(old_header, device)] = (inst, d)
            assert made[(old_header, 0)][1] == made[(old_header, 1)][1], (s, old_header)
            assert made[(old_header, 0)][1][:2] == (b"\x78\x01" if old_header else b"\x78\x9c")
        assert made[(False, 0)][1][2:] == made[(True, 0)][1][2:]
        if s == 9:   # a NIZK proof made over the digest of one path verifies over the digest of the other
            gens = P.NIZKGens(ctx, N, N, 10)
            tape = P.seed_scalar(b"tape", 9)
            host_inst, dev_inst = made[(False, 0)][0], made[(False, 1)][0]
            proofs = [P.NIZK.prove(ctx, i, i.vars, i.inputs, gens, b"nizk_digest", tape) for i in (host_inst, dev_inst)]
            assert proofs[0] == proofs[1]
            assert P.NIZK.verify_status(ctx, dev_inst, proofs[0], host_inst.inputs, gens, b"nizk_digest") == 1
            assert P.NIZK.verify_status(ctx, host_inst, proofs[1], dev_inst.inputs, gens, b"nizk_digest") == 1
            other = made[(True, 1)][0]           # the other header is another digest: the proof does not verify over it
            assert P.NIZK.verify_status(ctx, other, proofs[0], host_inst.inputs, gens, b"nizk_digest") == 0
            gens.free()
    finally:
        for inst, _ in made.values():
            inst.free()
