"""tdefl's coder on the device (spartan_amd/csrc/deflate_emit.hip; driven by spartan_amd/host/digest.cc): the block records and histograms of
sp_deflate_blocks are those of the host model (spz_deflate_blocks_host) element by element, the device-coded deflate (zlib_device(parse=2),
digest.device = 3) gives the sequential deflater's bytes, and an instance's digest — and so a NIZK proof — is the same whichever of the four
forms computed it. Inputs: the corpus of tests/deflate_corpus.py and the constructed cases of tests/deflate_token_cases.py and
tests/deflate_block_cases.py, all at most 200 000 bytes; segments of 49999 / 32768 / 65536 positions, and the lengths at which a block
boundary meets a segment's last token; tiles of 512 positions, groups of 2 tiles and chunks of 256 tokens, so that a 30 000-token block has
over a hundred chunks (tests/test_deflate_blocks.py shows on the CPU that every event of the block decisions occurs in these inputs)."""
import ctypes, random
import numpy as np
import pytest
from tests.helpers import *
from tests import deflate_corpus as dc
from tests import deflate_token_cases as tc
from tests import deflate_block_cases as bc
from tests.test_deflate_tokens import host_tokens
from tests.test_deflate_blocks import host_blocks, from_blocks, all_inputs, coinciding_segments, REC, HIST

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
def inputs(P):
    return all_inputs(P.H)


_HOST = {}


def _host(P, inputs, probes):
    """{name: (records, histograms, stream, stats of zlib_from_blocks)} of the host model and the sequential deflater, computed once"""
    if probes not in _HOST:
        _HOST[probes] = {}
        for name, x in inputs.items():
            tok, k, _ = host_tokens(P.H, x, probes)
            rec, hist, _ = host_blocks(P.H, tok, k, len(x))
            want = dc.zlib_probes(P.H, x, probes)
            z, st = from_blocks(P.H, x, rec, hist, tok, probes)
            assert z == want, name
            _HOST[probes][name] = (rec, hist, want, st, k)
    return _HOST[probes]


def _device_blocks(P, ctx, x, probes, **kw):
    rec, hist, nb = P.deflate_blocks(ctx, x, probes, **kw)
    return (np.frombuffer(rec, dtype=np.uint64, count=REC * nb).reshape(nb, REC), np.frombuffer(hist, dtype=np.uint16, count=HIST * nb).reshape(nb, HIST))


def _same_blocks(got, want, what):
    rec, hist = got
    k = min(len(rec), len(want[0]))
    bad = np.argwhere(rec[:k] != want[0][:k])
    assert len(bad) == 0, "records of %s: first difference in block %d, word %d: device %d, host %d" % (
        what, bad[0][0], bad[0][1], rec[bad[0][0]][bad[0][1]], want[0][bad[0][0]][bad[0][1]])
    bad = np.argwhere(hist[:k] != want[1][:k])
    assert len(bad) == 0, "histograms of %s: first difference in block %d, symbol %d: device %d, host %d" % (
        what, bad[0][0], bad[0][1], hist[bad[0][0]][bad[0][1]], want[1][bad[0][0]][bad[0][1]])
    assert len(rec) == len(want[0]), "%s: device has %d blocks, host %d (equal up to the shorter)" % (what, len(rec), len(want[0]))


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_blocks_equal_the_host_blocks(P, ctx, inputs, probes):
    want = _host(P, inputs, probes)
    for seg in bc.SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, x in inputs.items():
            if seg != bc.SEGMENTS[0] and len(x) <= 32768:
                continue   # one segment whatever the option says: run once
            _same_blocks(_device_blocks(P, ctx, x, probes, tile=tc.TILE, group=tc.GROUP), want[name], "%s, segment %d, %d probes" % (name, seg, probes))


def test_device_blocks_where_a_boundary_meets_a_seam(P, ctx, inputs):
    want = _host(P, inputs, 128)
    for name in ("text/200000", "random/200000", "text+random/30011"):
        for seg in coinciding_segments(P.H, inputs[name]):
            ctx.set_option("digest.segment", seg)
            _same_blocks(_device_blocks(P, ctx, inputs[name], 128, tile=tc.TILE, group=tc.GROUP), want[name], "%s, segment %d" % (name, seg))
            z, st = P.zlib_device(ctx, inputs[name], 128, parse=2, tile=tc.TILE, group=tc.GROUP, chunk=bc.CHUNK)
            assert z == want[name][2], (name, seg)


def _check_stats(st, x, seg, w, what):
    rec, _, _, hst, k = w
    assert st["emit"] == 1 and st["parse"] == 1 and st["device"] == 1 and st["segments"] == (len(x) + seg - 1) // seg, (what, st)
    assert st["tokens"] == 0 and st["lookups"] == 0 and st["tokens_coded"] == k, (what, st)          # no token came down
    assert st["blocks"] == len(rec) and st["stored_blocks"] == hst["stored"] and st["static_blocks"] == hst["static"], (what, st, hst)


@pytest.mark.parametrize("probes", dc.PROBES)
def test_device_coded_stream_equals_the_deflaters(P, ctx, inputs, probes):
    want = _host(P, inputs, probes)
    for seg in bc.SEGMENTS:
        ctx.set_option("digest.segment", seg)
        for name, x in inputs.items():
            if seg != bc.SEGMENTS[0] and len(x) <= 32768:
                continue
            z, st = P.zlib_device(ctx, x, probes, parse=2, tile=tc.TILE, group=tc.GROUP, chunk=bc.CHUNK)
            assert z == want[name][2], (name, seg, probes, len(z), len(want[name][2]))
            _check_stats(st, x, seg, want[name], (name, seg, probes))
    x = inputs["shape/2^9"]
    z, st = P.zlib_device(ctx, x, probes, old_header=True, parse=2, tile=tc.TILE, group=tc.GROUP, chunk=bc.CHUNK)
    assert z == dc.zlib_probes(P.H, x, probes, 1) and z[:2] == b"\x78\x01" and st["emit"] == 1
    z, st = P.zlib_device(ctx, x, probes, parse=1)
    assert z == want["shape/2^9"][2] and st["emit"] == 0 and st["parse"] == 1 and st["tokens"] > 0      # the form that ran is observed, not assumed


def test_device_coder_at_the_default_geometry_and_refused_chunks(P, ctx, inputs):
    want = _host(P, inputs, 128)
    ctx.set_option("digest.segment", 49999)
    for name in ("text/200000", "shape/2^12", "zeros/200000", "random/200000", "text+random/30011", "ends-at-check", "few-tokens", "zeros/0"):
        for old in (False, True):
            z, st = P.zlib_device(ctx, inputs[name], 128, old_header=old, parse=2)
            assert z == dc.zlib_probes(P.H, inputs[name], 128, int(old)), (name, old)
        _check_stats(st, inputs[name], 49999, want[name], name)
    for chunk in (255, 65537, 1):     # a chunk is a workgroup's worth of tokens at least
        with pytest.raises(P.SpartanHipError):
            P.zlib_device(ctx, inputs["text/65537"], 128, parse=2, chunk=chunk)


def _entries(rng, n, ncols):
    ent = [[(i, rng.randrange(ncols), rng.randrange(Q)) for i in range(n - 3 * k)] for k in range(3)]
    flat = [e for m in ent for e in m]
    u64 = ctypes.c_uint64
    return ([len(m) for m in ent], (u64 * len(flat))(*[e[0] for e in flat]), (u64 * len(flat))(*[e[1] for e in flat]),
            b"".join(e[2].to_bytes(32, "little") for e in flat))


def test_digest_is_the_same_in_all_four_forms(P, ctx):
    """an instance built by Instance.from_entries (no host copy of its entries): the digest under digest.device = 0, 1, 2 and 3, both headers"""
    N = 1 << 9
    ctx.set_option("digest.segment", 32768)     # 24 + 3 * 24 + 48 * 1527 = 73392 bytes: three segments
    nnz, rows, cols, vals = _entries(random.Random(11), N, N + 1 + 10)
    try:
        for old_header in (False, True):
            got = {}
            for device in (0, 1, 2, 3):
                ctx.set_option("digest.device", device)
                inst = P.Instance.from_entries(ctx, N, N, 10, nnz, rows, cols, bytearray(vals))
                inst.set_digest_header(old_header)
                got[device] = inst.digest()
                st = inst.digest_stats()
                assert st["device"] == (device != 0) and st["parse"] == (device >= 2) and st["emit"] == (device == 3), (device, st)
                if device == 3:
                    assert st["segments"] == 3 and st["tokens"] == 0 and st["tokens_coded"] > 0 and st["blocks"] >= 1, st
                inst.free()
            assert got[0] == got[1] == got[2] == got[3] and got[0][:2] == (b"\x78\x01" if old_header else b"\x78\x9c"), old_header
    finally:
        ctx.set_option("digest.device", 1)


def test_a_proof_made_under_the_device_coder_equals_one_made_under_the_host_parser(P, ctx):
    N = 1 << 9
    ctx.set_option("digest.segment", 49999)
    made = {}
    try:
        for device in (1, 3):
            ctx.set_option("digest.device", device)
            inst = P.Instance.produce_synthetic_r1cs(ctx, N, N, 10, seed=3)
            made[device] = (inst, inst.digest())
            assert inst.digest_stats()["emit"] == (device == 3)
        assert made[1][1] == made[3][1]
        gens = P.NIZKGens(ctx, N, N, 10)
        tape = P.seed_scalar(b"tape", 9)
        a, b = made[1][0], made[3][0]
        proofs = [P.NIZK.prove(ctx, i, i.vars, i.inputs, gens, b"nizk_digest", tape) for i in (a, b)]
        assert proofs[0] == proofs[1]
        assert P.NIZK.verify_status(ctx, b, proofs[0], a.inputs, gens, b"nizk_digest") == 1
        assert P.NIZK.verify_status(ctx, a, proofs[1], b.inputs, gens, b"nizk_digest") == 1
        gens.free()
    finally:
        ctx.set_option("digest.device", 1)
        for inst, _ in made.values():
            inst.free()
