"""The structured instances of tests/structured_cases.py on the CPU: each case's own predicates, the oracle's Instance::new / is_sat on it, the
oracle's SNARK and NIZK proofs with its own verifiers (accepted; rejected against a changed input), and the digests of those proofs and of
bincode(ComputationCommitment) against tests/golden/proof_digests.json ("structured"). ops_heavy_17 is too large for the oracle on every CPU run: only its predicates are checked here."""
import ctypes, json, os
import pytest
from tests.helpers import *
from tests import structured_cases as sc

GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests.json")))
SMALL = list(sc.SMALL)


@pytest.mark.parametrize("name", list(sc.CASES))
def test_case_reaches_what_it_claims(name):
    case = sc.get(name)                                       # the case function asserts its own predicates
    num_cons, num_vars, num_inputs, A, B, C, v, inputs = case
    assert len(v) == num_vars and len(inputs) == num_inputs
    assert all(0 <= r < num_cons and 0 <= c < num_vars + 1 + num_inputs and 0 <= x < Q for m in (A, B, C) for r, c, x in m)
    assert sc.failing_rows(case) == []
    st = sc.dense_stats(case)
    assert st["N"] == max(sc.next_pow2(n) for n in st["nnz"]) and st["hottest_cell_row"] == 0 and st["hottest_cell_col"] == 0
    if name in sc.SMALL:
        assert sc.CASES[name]() == case                       # seeded: a second build gives the same case (the large one is built once here;
                                                              # its worker processes rebuild it and must reach the oracle's proof of this build)


def test_regimes_are_reached():
    st = {name: sc.dense_stats(sc.get(name)) for name in sc.CASES}
    for name in ("ops_heavy", "ops_heavy_17"):
        assert st[name]["N"] == 32 * st[name]["cells"]        # num_ops much larger than num_mem_cells
    assert st["ops_heavy"]["max_read_ts_row"] > 4096 and st["ops_heavy"]["max_read_ts_col"] > 4096   # timestamps in the thousands
    assert len(set(st["ops_heavy"]["nnz"])) == 3 and len({sc.next_pow2(n) for n in st["ops_heavy"]["nnz"]}) == 3
    assert sc.padded_shape(sc.get("shifted")) == (64, 128, 28)
    assert st["long_row_hot_column"]["longest_row"] == 1025 and st["long_row_hot_column"]["N"] == st["long_row_hot_column"]["cells"]
    assert st["c_sparse"]["nnz"] == [32, 32, 3] and st["c_empty"]["nnz"] == [32, 32, 0]


@pytest.mark.parametrize("name", SMALL)
def test_oracle_accepts_the_instance_and_its_assignment(orc, name):
    case = sc.get(name)
    pk = sc.Packed(case)
    oi = pk.oracle_instance(orc)
    assert [orc.orc_instance_nnz(oi, ctypes.c_int(k)) for k in range(3)] == pk.nnz   # num_cons > 1: Instance::new adds no entries
    assert orc.orc_instance_is_sat(oi) == 1
    # the oracle's padding and shift against the case's own restatement of lib.rs:129-182
    ncp, nvp, shift = sc.padded_shape(case)
    tot = sum(pk.nnz)
    rows = (ctypes.c_uint64 * tot)(); cols = (ctypes.c_uint64 * tot)(); vals = (ctypes.c_uint64 * (4 * max(tot, 1)))()
    ov = (ctypes.c_uint64 * (4 * nvp))(); oin = (ctypes.c_uint64 * (4 * pk.num_inputs))()
    orc.orc_instance_export(oi, rows, cols, vals, ov, oin)
    ent = case[3] + case[4] + case[5]
    assert list(rows) == [e[0] for e in ent] and list(cols) == [e[1] + shift if e[1] >= pk.num_vars else e[1] for e in ent]
    assert from_mont_bulk(vals, tot) == [e[2] for e in ent]
    assert sc.oracle_bytes(orc, orc.orc_instance_shape_bincode, oi)[:24] == b"".join(x.to_bytes(8, "little") for x in (ncp, nvp, pk.num_inputs))
    orc.orc_instance_free(oi)
    w = list(case[6]); j = sc.BREAKING_VAR[name]
    w[j] = (w[j] + 1) % Q
    assert sc.failing_rows(case, vars_=w)
    ow = sc.Packed(case, vars_=w).oracle_instance(orc)
    assert orc.orc_instance_is_sat(ow) == 0                   # one variable changed
    orc.orc_instance_free(ow)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_proves_and_verifies(orc, name):
    orc.orc_set_threads(ctypes.c_int(1))
    run = sc.oracle_run(orc, name)
    st = sc.dense_stats(run.case)
    # bincode(ComputationCommitment) opens with num_cons, num_vars, num_inputs (padded), batch_size, num_ops = N, num_mem_cells = cells
    ncp, nvp, _ = sc.padded_shape(run.case)
    head = [int.from_bytes(run.commitment[8 * i:8 * i + 8], "little") for i in range(6)]
    assert head == [ncp, nvp, run.pk.num_inputs, 3, st["N"], st["cells"]]
    assert orc.orc_snark_verify(run.op, run.oi, run.og, run.oe, sc.SNARK_LABEL) == 1
    assert orc.orc_nizk_verify(run.onp, run.oi, run.ong, run.digest, sz(len(run.digest)), sc.NIZK_LABEL) == 1
    assert orc.orc_nizk_verify_bytes(run.nizk, sz(len(run.nizk)), run.oi, run.ong, run.digest, sz(len(run.digest)), sc.NIZK_LABEL) == 1
    assert orc.orc_nizk_verify(run.onp, run.oi, run.ong, b"other", sz(5), sc.NIZK_LABEL) == 0    # and the NIZK binds to its digest
    bad = run.wrong_inputs_instance().oracle_instance(orc)                                      # one input changed: both reject
    assert orc.orc_snark_verify(run.op, bad, run.og, run.oe, sc.SNARK_LABEL) == 0
    assert orc.orc_nizk_verify(run.onp, bad, run.ong, run.digest, sz(len(run.digest)), sc.NIZK_LABEL) == 0
    orc.orc_instance_free(bad)
    assert run.entry() == GOLD["structured"][name]


def test_golden_file_lists_exactly_the_small_cases():
    assert sorted(GOLD["structured"]) == sorted(SMALL)
    for e in GOLD["structured"].values():
        assert sorted(e) == ["commitment", "nizk", "snark"] and all(len(p["sha256"]) == 64 and p["len"] > 0 for p in e.values())
