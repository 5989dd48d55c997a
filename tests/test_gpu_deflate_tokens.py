"""tdefl's lazy parse on the device (the parse kernels of spartan_amd/csrc/deflate_match.hip; driven by spartan_amd/host/digest.cc): the tokens of
sp_deflate_tokens are those of the host model (spz_deflate_tokens_host) element by element, the device-parsed deflate gives the sequential
deflater's bytes, and an instance's digest — and so a NIZK proof — is the same whichever of the three forms computed it (digest.device = 0 the
host alone, 1 the device search and the host parser, 2 the device parse and the host token coder). Inputs: the corpus of
tests/deflate_corpus.py and the constructed cases of tests/deflate_token_cases.py, all at most 200 000 bytes; segments of 49999 / 32768 / 65536
positions as in tests/test_gpu_deflate_matches.py; tiles of 512 positions and groups of 2 tiles, so that a segment has about a hundred tiles
and fifty groups and every level of the hierarchy has many members (tests/test_deflate_tokens.py shows on the CPU that matches cross tile and
group boundaries and that held matches cross seams in these inputs)."""
import ctypes, random
import pytest
from tests.helpers import *
from tests import deflate_corpus as dc
from tests import deflate_token_cases as tc
from tests.test_deflate_tokens import host_tokens

pytestmark = pytest.mark.gpu


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
def inputs(orc):
    cases = dict(dc.build(orc))
    cases.update(tc.build())
    return cases


_HOST = {}


def _host(P, inputs, probes):
    """{name: (tokens, their number, stream)} of the host model and the sequential deflater at this probe count, computed once"""
    if probes not in _HOST:
        _HOST[probes] = {name: host_tokens(P.H, x, probes)[:2] + (dc.zlib_probes(P.H, x, probes),) for name, x in inputs.items()}
    return _HOST[probes]


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_tokens_equal_the_host_tokens(P, ctx, inputs, probes):
    want = _host(P, inputs, probes)
    held = fallbacks = 0
    for seg in tc.SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, x in inputs.items():
            if seg != tc.SEGMENTS[0] and len(x) <= 32768:
                continue   # one segment whatever the option says: run once
            tok, k, h, fb = P.deflate_tokens(ctx, x, probes, tile=tc.TILE, group=tc.GROUP)
            ref, kref, _ = want[name]
            p = dc.first_difference(tok, ref, min(k, kref))
            assert p is None, "tokens of %s, segment %d, %d probes: first difference at index %d: device %#x, host %#x" % (
                name, seg, probes, p, tok[p], ref[p])
            assert k == kref, "tokens of %s, segment %d, %d probes: device has %d, host %d (equal up to the shorter)" % (name, seg, probes, k, kref)
            held += h; fallbacks += fb
    assert held > 0 and fallbacks > 0, (held, fallbacks)   # segments were entered with a held match; look-ups were searched on the spot


def test_device_tokens_at_the_default_tile_and_group(P, ctx, inputs):
    want = _host(P, inputs, 128)
    ctx.set_option("digest.segment", 49999)
    for name in ("text/200000", "shape/2^12", "zeros+tail/70000", "lazy/70001"):
        tok, k, _, _ = P.deflate_tokens(ctx, inputs[name], 128)
        ref, kref, _ = want[name]
        p = dc.first_difference(tok, ref, min(k, kref))
        assert p is None and k == kref, (name, p, k, kref)
    for tile, group in ((511, 2), (4097, 2), (512, 1)):     # a tile holds the longest jump and fits the exits' LDS; a group has two tiles at least
        with pytest.raises(P.SpartanHipError):
            P.deflate_tokens(ctx, inputs["text/65537"], 128, tile=tile, group=group)


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_parsed_stream_equals_the_deflaters(P, ctx, inputs, probes):
    want = _host(P, inputs, probes)
    for seg in tc.SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, x in inputs.items():
            if seg != tc.SEGMENTS[0] and len(x) <= 32768:
                continue
            z, st = P.zlib_device(ctx, x, probes, parse=1, tile=tc.TILE, group=tc.GROUP)
            assert z == want[name][2], (name, seg, probes)
            assert st["parse"] == 1 and st["device"] == 1 and st["segments"] == (len(x) + seg - 1) // seg, (name, seg, st)
            assert st["tokens"] == want[name][1] and st["lookups"] == 0, (name, seg, st)
    x = inputs["shape/2^9"]
    z, st = P.zlib_device(ctx, x, probes, old_header=True, parse=1, tile=tc.TILE, group=tc.GROUP)
    assert z == dc.zlib_probes(P.H, x, probes, 1) and z[:2] == b"\x78\x01" and st["parse"] == 1
    z, st = P.zlib_device(ctx, x, probes, parse=0)
    assert z == want["shape/2^9"][2] and st["parse"] == 0 and st["lookups"] > 0       # the form that ran is observed, not assumed


def _entries(rng, n, ncols):
    ent = [[(i, rng.randrange(ncols), rng.randrange(Q)) for i in range(n - 3 * k)] for k in range(3)]
    flat = [e for m in ent for e in m]
    u64 = ctypes.c_uint64
    return ([len(m) for m in ent], (u64 * len(flat))(*[e[0] for e in flat]), (u64 * len(flat))(*[e[1] for e in flat]),
            b"".join(e[2].to_bytes(32, "little") for e in flat))


def test_digest_is_the_same_in_all_three_forms(P, ctx):
    """an instance built by Instance.from_entries (no host copy of its entries): the digest under digest.device = 0, 1 and 2, both headers"""
    N = 1 << 9
    ctx.set_option("digest.segment", 32768)     # 24 + 3 * 24 + 48 * 1527 = 73392 bytes: three segments
    nnz, rows, cols, vals = _entries(random.Random(11), N, N + 1 + 10)
    try:
        for old_header in (False, True):
            got = {}
            for device in (0, 1, 2):
                ctx.set_option("digest.device", device)
                inst = P.Instance.from_entries(ctx, N, N, 10, nnz, rows, cols, bytearray(vals))
                inst.set_digest_header(old_header)
                got[device] = inst.digest()
                st = inst.digest_stats()
                assert st["device"] == (device != 0) and st["parse"] == (device == 2), (device, st)
                if device == 2:
                    assert st["segments"] == 3 and st["tokens"] > 0 and st["lookups"] == 0, st
                inst.free()
            assert got[0] == got[1] == got[2] and got[0][:2] == (b"\x78\x01" if old_header else b"\x78\x9c"), old_header
    finally:
        ctx.set_option("digest.device", 1)


def test_a_proof_made_under_one_form_verifies_under_the_other(P, ctx):
    N = 1 << 9
    ctx.set_option("digest.segment", 49999)
    made = {}
    try:
        for device in (1, 2):
            ctx.set_option("digest.device", device)
            inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=3)
            made[device] = (inst, inst.digest())
            assert inst.digest_stats()["parse"] == (device == 2)
        assert made[1][1] == made[2][1]
        gens = P.NIZKGens(ctx, N, N, 10)
        tape = P.seed_scalar(b"tape", 9)
        a, b = made[1][0], made[2][0]
        proofs = [P.NIZK.prove(ctx, i, i.vars, i.inputs, gens, b"nizk_digest", tape) for i in (a, b)]
        assert proofs[0] == proofs[1]
        assert P.NIZK.verify_status(ctx, b, proofs[0], a.inputs, gens, b"nizk_digest") == 1
        assert P.NIZK.verify_status(ctx, a, proofs[1], b.inputs, gens, b"nizk_digest") == 1
        gens.free()
    finally:
        ctx.set_option("digest.device", 1)
        for inst, _ in made.values():
            inst.free()
