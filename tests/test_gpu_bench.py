"""bench.py's plain run (no --full) and --dump-outputs: the headline keys, --steps as the number of timed steps, and the dumped
proof of the last timed step equal to the oracle's proof of the same seeded instance and tape, run after run."""
import ctypes, json, os, subprocess, sys

import numpy as np
import pytest

from tests.helpers import ROOT, sz, vp

pytestmark = pytest.mark.gpu


def _bench(outdir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log2-cons", "10", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(outdir)] + list(extra), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(os.path.join(str(outdir), "proof.npy"))


def test_plain_run_dumps_the_oracle_proof(tmp_path, orc):
    line, got = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["unit"] == "constraints/s" and line["higher_is_better"] is True
    assert line["value"] == pytest.approx((1 << 10) / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert "roofline" not in line and "cpu_baseline" not in line and "throughput_concurrent" not in line   # --full only
    assert got.dtype == np.float64 and got.ndim == 1 and len(got) == line["config"]["proof_bytes"]
    proof = got.astype(np.uint8).tobytes()
    assert (got == np.frombuffer(proof, dtype=np.uint8)).all()
    # the oracle's proof of bench.py's rank-0 instance (seed 0) and tape (seed 100)
    N = 1 << 10
    inst = vp(orc.orc_instance_synthetic(sz(N), sz(N), sz(10), ctypes.c_uint64(0)))
    g = vp(orc.orc_snark_gens_new(sz(N), sz(N), sz(10), sz(N)))
    e = vp(orc.orc_snark_encode(inst, g))
    seed = (ctypes.c_uint64 * 4)()
    orc.orc_seed_scalar(b"tape", ctypes.c_uint64(100), seed)
    p = vp(orc.orc_snark_prove(inst, g, e, b"snark_example", seed, None))
    n = orc.orc_proof_bytes(p, None, sz(0)); b = (ctypes.c_uint8 * n)(); orc.orc_proof_bytes(p, b, sz(n))
    orc.orc_proof_free(p); orc.orc_encode_free(e); orc.orc_snark_gens_free(g); orc.orc_instance_free(inst)
    assert proof == bytes(b)
    # same arguments, same outputs
    line2, got2 = _bench(tmp_path / "b")
    assert (got2 == got).all() and line2["config"]["proof_sha256"] == line["config"]["proof_sha256"]
