"""CPU-side checks of Commitment.encode's boundary: the host library exports the entry points, the Python class has the methods, and a call
without a context fails with a message instead of crashing."""
import ctypes


def test_host_library_exports_the_entry_points():
    from spartan_amd import prover
    for f in ("spz_commitment_encode", "spz_commitment_serialize", "spz_commitment_resident_bytes"):
        assert hasattr(prover.H, f), f


def test_commitment_class_has_the_methods():
    from spartan_amd import prover
    for m in ("encode", "serialize", "resident_bytes", "load", "free"):
        assert callable(getattr(prover.Commitment, m)), m


def test_encode_without_a_context_is_an_error_not_a_crash():
    from spartan_amd import prover
    H = prover.H
    for args in ((None, None, None), (None, ctypes.c_void_p(8), ctypes.c_void_p(8))):
        assert not H.spz_commitment_encode(*args)
        assert b"spz_commitment_encode" in H.spz_last_error()
    assert H.spz_commitment_serialize(None, None, ctypes.c_size_t(0)) == 0
    assert H.spz_commitment_resident_bytes(None) == 0
    class Null:
        h = None
    try:
        prover.Commitment.encode(Null, Null, Null)
    except prover.SpartanHipError as e:
        assert "Commitment.encode failed" in str(e)
    else:
        raise AssertionError("no error")
