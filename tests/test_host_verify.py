"""CPU-side pieces of NIZK::verify (no GPU): sp_host_msm_var, the few-term variable-base combination of the verifier, against the oracle's
orc_pt_msm; and the bincode parser of untrusted proof bytes (spz_nizk_parse_probe: parse and serialise again) on oracle proofs and on
damaged copies of them."""
import ctypes, random, time
import pytest
from tests.helpers import *
from tests import msm_var_cases as M

SP_EINVAL, SP_EPOINT = -1, -4


@pytest.fixture(scope="module")
def lib():
    from spartan_amd import capi
    return capi.lib


def host_msm(lib, pts, scalars):
    out = (ctypes.c_uint8 * 32)()
    rc = lib.sp_host_msm_var(b"".join(pts), mont_array(scalars), sz(len(pts)), out)
    return rc, bytes(out)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 21, 43, 64])
def test_host_msm_var_matches_oracle(lib, orc, n):
    rng = random.Random(n)
    pts = M.points(orc, n)
    for kind in ("uniform", "sparse", "small", "edge"):
        S = rand_scalars(rng, n, kind)
        rc, got = host_msm(lib, pts, S)
        assert rc == 0 and got == M.oracle_msm(orc, pts, S), (n, kind)


@pytest.mark.parametrize("n", [5, 64])
def test_host_msm_var_named_cases(lib, orc, n):
    rng = random.Random(100 + n)
    for name, pts, S in M.named_cases(orc, rng, n):
        rc, got = host_msm(lib, pts, S)
        assert rc == 0 and got == M.oracle_msm(orc, pts, S), (name, n)
        if name in ("all_zero", "only_a_pair_of_negatives"):
            assert got == M.IDENTITY, name


def test_host_msm_var_errors(lib, orc):
    from tests.test_oracle_pins import RFC_BAD
    pts = M.points(orc, 65)
    S = [3] * 65
    assert host_msm(lib, pts, S)[0] == SP_EINVAL                      # n = 65
    out = (ctypes.c_uint8 * 32)()
    assert lib.sp_host_msm_var(b"".join(pts), mont_array(S), sz(0), out) == SP_EINVAL
    assert lib.sp_host_msm_var(None, mont_array(S), sz(2), out) == SP_EINVAL
    assert lib.sp_host_msm_var(b"".join(pts), None, sz(2), out) == SP_EINVAL
    assert lib.sp_host_msm_var(b"".join(pts), mont_array(S), sz(2), None) == SP_EINVAL
    for enc in RFC_BAD:
        for where in (0, 2, 4):
            bad = list(pts[:5]); bad[where] = bytes.fromhex(enc)
            assert host_msm(lib, bad, S[:5])[0] == SP_EPOINT, (enc, where)


# ---- the parser
@pytest.fixture(scope="module")
def H():
    from spartan_amd import prover
    return prover.H


def oracle_nizk_proof(orc, s, seed):
    N = 1 << s
    ni = 10 if N > 16 else 1
    oi = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(ni), ctypes.c_uint64(seed)))
    og = vp(orc.orc_nizk_gens_new(sz(N), sz(N), sz(ni)))
    tape = (ctypes.c_uint64 * 4)()
    orc.orc_seed_scalar(b"tape", ctypes.c_uint64(seed), tape)
    op = vp(orc.orc_nizk_prove(oi, og, b"digest", sz(6), b"nizk_example", tape, None))
    n = orc.orc_proof_bytes(op, None, sz(0)); b = (ctypes.c_uint8 * n)(); orc.orc_proof_bytes(op, b, sz(n))
    orc.orc_proof_free(op); orc.orc_nizk_gens_free(og); orc.orc_instance_free(oi)
    return bytes(b)


@pytest.fixture(scope="module")
def proofs(orc):
    return {s: oracle_nizk_proof(orc, s, seed) for s, seed in ((1, 0), (4, 2), (10, 4))}


def probe(H, b):
    out = (ctypes.c_uint8 * (len(b) + 64))()
    n = H.spz_nizk_parse_probe(bytes(b), sz(len(b)), out, sz(len(out)))
    return n, bytes(out[:max(n, 0)])


@pytest.mark.parametrize("s", [1, 4, 10])
def test_parse_round_trips_oracle_proofs(H, proofs, s):
    n, again = probe(H, proofs[s])
    assert n == len(proofs[s]) and again == proofs[s]


def test_parse_refuses_every_truncation_and_trailing_bytes(H, proofs):
    p = proofs[1]
    for k in range(len(p)):
        assert probe(H, p[:k])[0] == -1, k
    assert probe(H, p + b"\x00")[0] == -1


def _vec_length_offsets(p):
    """offsets of the u64 length fields of an NIZK proof at 2^s, from the struct layout (r1csproof.rs:21-37): comm_vars, then per sum-check
    comm_polys, comm_evals, proofs and each proof's z; L_vec, R_vec; rx, ry"""
    u64 = lambda o: int.from_bytes(p[o:o + 8], "little")
    offs, o = [], 0
    def vec(elem):
        nonlocal o
        offs.append(o); k = u64(o); o += 8 + elem * k
    vec(32)
    def zksc():
        nonlocal o
        vec(32); vec(32)
        offs.append(o); k = u64(o); o += 8
        for _ in range(k):
            o += 64; vec(32); o += 64
    zksc()
    o += 4 * 32 + 96 + 96 + 5 * 32 + 64
    zksc()
    o += 32
    vec(32); vec(32)
    o += 64 + 64 + 64
    vec(32); vec(32)
    assert o == len(p)
    return offs


def test_parse_refuses_huge_lengths_without_allocating(H, proofs):
    p = proofs[4]
    offs = _vec_length_offsets(p)
    assert len(offs) >= 12
    t0 = time.perf_counter()
    for o in offs:
        for huge in (1 << 60, (1 << 64) - 1, (len(p) // 32) + 1):
            bad = p[:o] + huge.to_bytes(8, "little") + p[o + 8:]
            assert probe(H, bad)[0] == -1, (o, huge)
    assert time.perf_counter() - t0 < 2.0     # 2^60 elements were never allocated


def test_parse_refuses_unreduced_scalars(H, proofs):
    p = proofs[4]
    tail = len(p) - 32                          # the last scalar of ry
    for v in (Q, Q + 1, (1 << 256) - 1):
        assert probe(H, p[:tail] + v.to_bytes(32, "little"))[0] == -1
    assert probe(H, p[:tail] + (Q - 1).to_bytes(32, "little"))[0] == len(p)
    # a scalar inside the R1CSProof: proof_eq_sc_phase2.z sits right before rx
    ry_len = int.from_bytes(p[len(p) - 32 * 5 - 8:len(p) - 32 * 5], "little")
    assert ry_len == 5
    z_off = len(p) - (8 + 32 * 5) - (8 + 32 * 4) - 32
    assert probe(H, p[:z_off] + Q.to_bytes(32, "little") + p[z_off + 32:])[0] == -1
