"""Shared inputs of the variable-base MSM tests (tests/test_gpu_msm_var.py: sp_msm_var on the device; tests/test_host_verify.py:
sp_host_msm_var on the CPU): seeded points from the oracle's one-way map and the named edge cases, each compared byte for byte with
the oracle's orc_pt_msm (oracle/capi_prims.cc:34)."""
import ctypes, hashlib
from tests.helpers import Q, mont_array, sz

IDENTITY = bytes(32)
_POINTS = {}


def points(orc, n, seed=0):
    """n encoded points: orc_pt_from_uniform_bytes over a SHAKE256 stream keyed by the seed (computed once per seed, extended on demand)"""
    have = _POINTS.setdefault(seed, [])
    if len(have) < n:
        stream = hashlib.shake_256(b"msm_var test points %d" % seed).digest(64 * n)
        out = (ctypes.c_uint8 * 32)()
        for i in range(len(have), n):
            orc.orc_pt_from_uniform_bytes(stream[64 * i:64 * i + 64], out)
            have.append(bytes(out))
    return have[:n]


def negate(orc, p):
    """-P: (q - 1) * P from the oracle"""
    out = (ctypes.c_uint8 * 32)()
    assert orc.orc_pt_mul_bytes((Q - 1).to_bytes(32, "little"), p, out) == 1
    return bytes(out)


def oracle_msm(orc, pts, scalars):
    out = (ctypes.c_uint8 * 32)()
    assert orc.orc_pt_msm(mont_array(scalars), b"".join(pts), sz(len(pts)), out) == 1
    return bytes(out)


def named_cases(orc, rng, n):
    """[(name, points, scalars)] at size n >= 4"""
    base = points(orc, n, seed=1)
    P = base[0]
    k = rng.randrange(1, Q)
    adjacent = list(base); adjacent[2] = P; adjacent[3] = negate(orc, P)
    distant = list(base); distant[0] = P; distant[n - 1] = negate(orc, P)
    eq = [rng.randrange(Q) for _ in range(n)]
    eq_adj = list(eq); eq_adj[2] = eq_adj[3] = k
    eq_dist = list(eq); eq_dist[0] = eq_dist[n - 1] = k
    with_id = list(base); with_id[1] = IDENTITY; with_id[n // 2] = IDENTITY
    return [
        ("all_zero", base, [0] * n),
        ("one_point_repeated", [P] * n, [1] * n),
        ("negatives_adjacent", adjacent, eq_adj),
        ("negatives_distant", distant, eq_dist),
        ("only_a_pair_of_negatives", [P, negate(orc, P)] * (n // 2) + [IDENTITY] * (n % 2), [k] * n),
        ("identity_among_inputs", with_id, [rng.randrange(Q) for _ in range(n)]),
        ("q_minus_1_everywhere", base, [Q - 1] * n),
    ]
