"""The structured instances of tests/structured_cases.py through the library, byte for byte against the oracle: Instance::is_sat,
SNARK::encode (commitment and decommitment), SNARK::prove, NIZK::prove, NIZK::verify and the shape serialisation behind the digest.
They reach what no synthetic instance does: num_ops = 32 num_mem_cells, three matrices of different nnz (thousands of (0, 0, 0) padding
entries, all of them reads of cell 0), shifted constant and input columns with real structure, and a matrix without any entry (c_empty:
sp_sparse_upload keeps one-element buffers for it, sp_sparse_entry_index / _values write padding only, every kernel's loop over its
entries is empty). The small cases are also held against the committed digests of tests/golden/proof_digests.json; ops_heavy_17 must
give the oracle's proof under the settings whose code paths depend on table lengths, one fresh process each."""
import ctypes, hashlib, json, os, subprocess, sys, time, zlib
import pytest
from tests.helpers import *
from tests import structured_cases as sc

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_digests.json")))["structured"]
SMALL = list(sc.SMALL)
LARGE = "ops_heavy_17"


@pytest.fixture(scope="module")
def P():
    from spartan_amd import prover
    return prover


@pytest.fixture(scope="module")
def ctx(P):
    c = P.Ctx(0)
    yield c
    c.close()


class Side:
    """the library's side of one case next to the oracle's (sc.OracleRun, computed once per process): instance, generators, SNARK::encode and
    both proofs over the case's tape. The digest is read before set_digest(b"<case name>") replaces it."""
    def __init__(self, P, ctx, orc, name):
        orc.orc_set_threads(ctypes.c_int(16 if name == LARGE else 1))
        self.P, self.ctx, self.name = P, ctx, name
        self.run = run = sc.oracle_run(orc, name)
        self.pk = pk = run.pk
        self.inst = P.Instance.new(ctx, pk.num_cons, pk.num_vars, pk.num_inputs, pk.nnz, pk.rows, pk.cols, pk.vals)
        self.computed_digest = self.inst.digest()
        self.inst.set_digest(run.digest)
        self.tape = P.seed_scalar(b"tape", sc.TAPE_SEED[name])
        assert bytes(self.tape) == bytes(run.tape)
        self.gens = P.SNARKGens(ctx, *run.gens_args)
        self.ngens = P.NIZKGens(ctx, *run.gens_args[:3])
        self.enc = P.SNARK.encode(ctx, self.inst, self.gens)
        self.snark = P.SNARK.prove(ctx, self.inst, self.enc, pk.vars, pk.inputs, self.gens, sc.SNARK_LABEL, self.tape)
        self.nizk = P.NIZK.prove(ctx, self.inst, pk.vars, pk.inputs, self.ngens, sc.NIZK_LABEL, self.tape)

    def free(self):
        self.enc.free(); self.ngens.free(); self.gens.free(); self.inst.free()


@pytest.fixture(scope="module")
def sides(P, ctx, orc):
    made = {}
    def get(name):
        if name not in made:
            made[name] = Side(P, ctx, orc, name)
        return made[name]
    yield get
    for s in made.values():
        s.free()


def _same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got != want:
        first = next(i for i in range(len(got)) if got[i] != want[i])
        pytest.fail(f"{what}: first differing byte at offset {first} of {len(got)}")


def _check_is_sat(P, ctx, s):
    pk, case = s.pk, s.run.case
    w = list(case[6]); j = sc.BREAKING_VAR[s.name]
    w[j] = (w[j] + 1) % Q
    truth = sc.failing_rows(case, vars_=w)
    assert truth
    bad = mont_bulk(w)
    for good_src, bad_src in ((pk.vars, bad), (P.VarsAssignment(ctx, pk.vars), P.VarsAssignment(ctx, bad))):   # host limbs, then resident
        assert s.inst.is_sat(good_src, pk.inputs) is True
        assert s.inst.is_sat(bad_src, pk.inputs) is False
        rep = s.inst.check(bad_src, pk.inputs, max_rows=len(truth))
        assert rep.violated == len(truth) and rep.rows == truth
        if isinstance(good_src, P.VarsAssignment):
            good_src.free(); bad_src.free()


def _check_encode(orc, s, decommitment=True):
    _same(s.enc.serialize_commitment(), s.run.commitment, "bincode(ComputationCommitment)")
    if decommitment:   # the timestamps, the comb_ops / comb_mem layout and the padding entries, element by element
        _same(s.enc.serialize_decommitment(), sc.oracle_bytes(orc, orc.orc_decommitment_bincode, s.run.oe), "bincode(ComputationDecommitment)")


def _check_proofs(P, ctx, orc, s):
    run, pk = s.run, s.pk
    l0 = run.snark_sat_len
    _same(s.snark[:l0], run.snark[:l0], "SNARK r1cs_sat_proof")     # splits the prover: the satisfiability part, then the rest
    _same(s.snark, run.snark, "SNARK proof")
    assert orc.orc_snark_verify(run.op, run.oi, run.og, run.oe, sc.SNARK_LABEL) == 1   # run.op holds the very bytes just compared
    _same(s.nizk, run.nizk, "NIZK proof")
    d = run.digest
    assert orc.orc_nizk_verify_bytes(s.nizk, sz(len(s.nizk)), run.oi, run.ong, d, sz(len(d)), sc.NIZK_LABEL) == 1
    assert P.NIZK.verify_status(ctx, s.inst, s.nizk, pk.inputs, s.ngens, sc.NIZK_LABEL) == 1
    assert P.NIZK.verify_status(ctx, s.inst, run.nizk, pk.inputs, s.ngens, sc.NIZK_LABEL) == 1
    assert P.NIZK.verify_status(ctx, s.inst, s.nizk, run.wrong_inputs(), s.ngens, sc.NIZK_LABEL) == 0   # one input changed
    assert P.NIZK.verify_status(ctx, s.inst, run.nizk, run.wrong_inputs(), s.ngens, sc.NIZK_LABEL) == 0


def _check_shape(orc, s):
    """the product's own shape serialisation (Instance::shape_bincode under the in-tree deflater) with unequal nnz and shifted columns"""
    _same(zlib.decompress(s.computed_digest), sc.oracle_bytes(orc, orc.orc_instance_shape_bincode, s.run.oi), "bincode(R1CSShape)")


@pytest.mark.parametrize("name", SMALL)
def test_is_sat_from_host_limbs_and_resident(P, ctx, sides, name):
    _check_is_sat(P, ctx, sides(name))


@pytest.mark.parametrize("name", SMALL)
def test_encode_commitment_and_decommitment_match_oracle(orc, sides, name):
    s = sides(name)
    st = sc.dense_stats(s.run.case)
    assert len(s.enc.comm(0)) // 32 == 1 << ((sc.next_pow2(15 * st["N"]).bit_length() - 1) // 2)   # rows of the comb_ops commitment
    _check_encode(orc, s)


@pytest.mark.parametrize("name", SMALL)
def test_snark_and_nizk_bytes_match_oracle_and_verify(P, ctx, orc, sides, name):
    _check_proofs(P, ctx, orc, sides(name))


@pytest.mark.parametrize("name", SMALL)
def test_computed_digest_inflates_to_the_oracle_shape(orc, sides, name):
    _check_shape(orc, sides(name))


@pytest.mark.parametrize("name", SMALL)
def test_committed_digests(sides, name):
    s = sides(name)
    sha = lambda b: hashlib.sha256(b).hexdigest()
    g = GOLD[name]
    l0 = g["snark"]["sat_len"]
    assert (len(s.snark), sha(s.snark[:l0]), sha(s.snark[l0:]), sha(s.snark)) == (g["snark"]["len"], g["snark"]["sat_sha256"], g["snark"]["rest_sha256"], g["snark"]["sha256"])
    assert (len(s.nizk), sha(s.nizk)) == (g["nizk"]["len"], g["nizk"]["sha256"])
    cb = s.enc.serialize_commitment()
    assert (len(cb), sha(cb)) == (g["commitment"]["len"], g["commitment"]["sha256"])


def test_ops_heavy_17_matches_oracle(P, ctx, orc, sides):
    """2^17 ops over 2^12 cells in one process: everything the small cases check, the decommitment (a 2^21-element table, downloaded and
    compared whole) included."""
    t0 = time.time()
    s = sides(LARGE)
    t1 = time.time()
    _check_is_sat(P, ctx, s)
    _check_encode(orc, s)
    _check_proofs(P, ctx, orc, s)
    _check_shape(orc, s)
    print("ops_heavy_17: oracle and device sides %.1f s, checks %.1f s" % (t1 - t0, time.time() - t1))


# the settings whose code paths depend on table lengths: here the ops circuits are 2^17 long while the mem circuits (2^12) are on the
# short-table and host-tail paths — with the synthetic instance of test_every_ab_switch_gives_the_same_proof it is the other way round
LENGTH_SETTINGS = [{}, {"spark.eq_factor": 0}, {"spark.hash_fuse": 0}, {"spark.prod_layer2": 0},
                   {"sumcheck.double_round_max_len": 0, "sumcheck.host_tail": 0}, {"msm.form": 3},
                   {"msm.lds_bits": 10, "msm.form": 1}]


@pytest.mark.parametrize("setting", LENGTH_SETTINGS, ids=lambda st: ",".join("%s=%d" % kv for kv in st.items()) or "default")
def test_ops_heavy_17_under_length_dependent_settings(orc, setting):
    orc.orc_set_threads(ctypes.c_int(16))
    want = hashlib.sha256(sc.oracle_run(orc, LARGE).snark).hexdigest()
    e = dict(os.environ, SPARTAN_OPTIONS=options_env(**{k.replace(".", "__"): v for k, v in setting.items()}))
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_worker.py"), "17", str(sc.TAPE_SEED[LARGE]), LARGE], env=e,
                       capture_output=True, text=True, timeout=600)
    print("switch_worker.py 17 %d %s %s: %.1f s" % (sc.TAPE_SEED[LARGE], LARGE, setting, time.time() - t0))
    assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("PROOF_SHA256")]
    assert line and line[0].split()[1] == want, (setting, line)
