"""The parsers of SNARK::verify on untrusted bytes, without a GPU: SNARK::deserialize (spz_snark_reserialize: parse, serialise again) and
ComputationCommitment::deserialize (spz_commitment_reserialize) on the oracle's bytes and on damaged copies of them. Every damaged copy is
-1 and the process lives; every Vec length of the proof, outer and nested, is replaced in turn by 2^63 and by one more than fits."""
import ctypes, time
import pytest
from tests.helpers import *
from tests.snark_layout import Layout


@pytest.fixture(scope="module")
def H():
    from spartan_amd import prover
    return prover.H


def _bytes(orc, fn, h):
    n = fn(h, None, sz(0)); b = (ctypes.c_uint8 * n)(); fn(h, b, sz(n))
    return bytes(b)


def oracle_snark(orc, s, seed):
    """(proof bytes, commitment bytes) of the oracle's SNARK over a synthetic instance at 2^s, as tests/test_oracle_pins.py makes them"""
    N = 1 << s
    ni = 10 if N > 16 else 1
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    og = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(ni), sz(N)))
    oe = vp(orc.orc_snark_encode(oi, og))
    tape = u64x4(); orc.orc_seed_scalar(b"tape", ctypes.c_uint64(seed), tape)
    op = vp(orc.orc_snark_prove(oi, og, oe, b"snark_example", tape, None))
    proof, comm = _bytes(orc, orc.orc_proof_bytes, op), _bytes(orc, orc.orc_commitment_bincode, oe)
    orc.orc_proof_free(op); orc.orc_encode_free(oe); orc.orc_snark_gens_free(og); orc.orc_instance_free(oi)
    return proof, comm


@pytest.fixture(scope="module")
def made(orc):
    return {s: oracle_snark(orc, s, seed) for s, seed in ((1, 0), (4, 2), (6, 4))}


def reser(H, b, fn="spz_snark_reserialize"):
    out = (ctypes.c_uint8 * (len(b) + 64))()
    n = getattr(H, fn)(bytes(b), sz(len(b)), out, sz(len(out)))
    return n, bytes(out[:max(n, 0)])


@pytest.mark.parametrize("s", [1, 4, 6])
def test_oracle_proofs_survive_byte_for_byte(H, made, s):
    p = made[s][0]
    n, again = reser(H, p)
    assert n == len(p) and again == p


@pytest.mark.parametrize("s", [1, 4, 6])
def test_truncated_extended_and_doubled_proofs_are_malformed(H, made, s):
    p = made[s][0]
    for k in (0, 7, 8, len(p) // 2, len(p) - 1):
        assert reser(H, p[:k])[0] == -1, k
    assert reser(H, p + b"\x00")[0] == -1
    assert reser(H, p + p)[0] == -1
    assert reser(H, p)[0] == len(p)


def test_every_prefix_of_the_smallest_proof_is_malformed(H, made):
    p = made[1][0]
    for k in range(0, len(p), 5):
        assert reser(H, p[:k])[0] == -1, k


@pytest.mark.parametrize("s", [1, 4, 6])
def test_every_vec_length_in_turn_huge_or_one_too_many(H, made, s):
    p = made[s][0]
    lay = Layout(p)
    names = {n for _, _, n in lay.lengths}
    # the nested ones are there: Vec<LayerProofBatched>, Vec<CompressedUniPoly> and a CompressedUniPoly's own Vec<Scalar> (from the second layer on)
    assert "proof_ops.proof" in names and "proof_ops.proof[0].compressed_polys" in names and "proof_mem.proof[1].compressed_polys[0]" in names
    assert len(lay.lengths) >= 50      # 50 at 2^1, more with every sum-check round and layer
    t0 = time.perf_counter()
    for off, min_elem, name in lay.lengths:
        fits = (len(p) - (off + 8)) // min_elem
        for k in (1 << 63, fits + 1):
            assert reser(H, p[:off] + k.to_bytes(8, "little") + p[off + 8:])[0] == -1, (name, k)
    assert time.perf_counter() - t0 < 5.0     # 2^63 elements were never allocated


@pytest.mark.parametrize("s", [1, 6])
def test_unreduced_scalars_are_malformed(H, made, s):
    p = made[s][0]
    lay = Layout(p)
    scalars = [(n, o) for n, (o, kind) in lay.fields.items() if kind == "scalar"]
    assert len(scalars) > 40
    for name, o in scalars:
        assert reser(H, p[:o] + Q.to_bytes(32, "little") + p[o + 32:])[0] == -1, name
    name, o = scalars[-1]
    assert reser(H, p[:o] + ((1 << 256) - 1).to_bytes(32, "little") + p[o + 32:])[0] == -1
    assert reser(H, p[:o] + (Q - 1).to_bytes(32, "little") + p[o + 32:])[0] == len(p)


# ---- ComputationCommitment: six u64 (num_cons, num_vars, num_inputs, batch_size, num_ops, num_mem_cells), then the two share vectors
@pytest.mark.parametrize("s", [1, 4, 6])
def test_commitment_round_trips(H, made, s):
    c = made[s][1]
    n, again = reser(H, c, "spz_commitment_reserialize")
    assert n == len(c) and again == c


def test_damaged_commitments_are_malformed(H, made):
    c = made[6][1]
    rs = lambda b: reser(H, b, "spz_commitment_reserialize")[0]
    u64 = lambda o: int.from_bytes(c[o:o + 8], "little")
    put = lambda o, v: c[:o] + v.to_bytes(8, "little") + c[o + 8:]
    n_ops = u64(48)
    off_mem = 56 + 32 * n_ops
    n_mem = u64(off_mem)
    assert u64(24) == 3 and n_ops == 32 and n_mem == 16 and off_mem + 8 + 32 * n_mem == len(c)   # 2^6: comb_ops 2^10 entries, comb_mem 2^8
    for k in (0, 7, 8, 47, 48, 56, len(c) // 2, len(c) - 1):
        assert rs(c[:k]) == -1, k
    assert rs(c + b"\x00") == -1 and rs(c + c) == -1
    assert rs(put(24, 2)) == -1 and rs(put(24, 4)) == -1                        # batch_size
    for o in (48, off_mem):                                                     # the two lengths
        for k in (1 << 63, (len(c) - o - 8) // 32 + 1, 0):
            assert rs(put(o, k)) == -1, (o, k)
    # share counts that parse but are not what encode gives: not a power of two; not the size num_ops / num_mem_cells call for; none; too many
    assert rs(put(48, 31)[:56 + 32 * 31] + c[off_mem:]) == -1
    assert rs(put(48, 16)[:56 + 32 * 16] + c[off_mem:]) == -1
    assert rs(c[:off_mem] + (4).to_bytes(8, "little") + c[off_mem + 8:off_mem + 8 + 32 * 4]) == -1
    assert rs(put(32, u64(32) * 4)) == -1 and rs(put(40, u64(40) * 4)) == -1   # num_ops, num_mem_cells against the share counts
    assert rs(put(32, 0)) == -1 and rs(put(40, 0)) == -1 and rs(put(0, 0)) == -1 and rs(put(8, 0)) == -1
    big = (1 << 17).to_bytes(8, "little")
    assert rs(c[:32] + (1 << 30).to_bytes(8, "little") + c[40:48] + big + c[56:88] * (1 << 17) + c[off_mem:]) == -1   # 2^17 shares > 65536
    assert rs(c) == len(c)
